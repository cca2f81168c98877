// lora_rows.h -- LoRA, the one path: every token row of a step names the adapter it runs.  Per-request adapters
// (mi_engine_set_adapter_lora / mi_kv_set_row_adapter) give the rows of one step different adapters; the engine-wide adapter
// (mi_engine_set_lora) is a private column of the same table that every row names.  Launch interface of lora_rows.hip; beside
// kernels.h, so that no linear kernel's header changes.
//
// Every fused matrix of a block that some resident adapter covers owns a device table [part][LORA_TABLE_COLS] of AdapterPart;
// a step uploads row_adapter[token row] (-1: none) and each adapted linear runs
//   launch_lora_down_by_row    t[m][part][0..rank) = x_m A of the row's adapter (x and its RMSNorm staged once per row)
//   the base linear            plain store, no LoRA term
//   launch_lora_up_add_by_row  y[m][row0 + n] = R(y + R(scale . z)) per row, optionally followed by h[m][n] = R(h + y')
//
// DoRA (mi_engine_set_dora / mi_engine_set_adapter_dora): an entry may carry a per-column gain g[n] = m[n] / ||W[n] + scale (A B)^T[n]||,
// computed once when the entry is set (launch_dora_gain) and kept as unrounded float32.  The up-add then ends an adapted row
// with y' = R(R(g[n]) . y') ahead of the residual add -- in an instantiation of its own, launched only for a table that
// holds a gain (LoraRowsCall::gain); rows whose entry has none take no multiplication there.
#pragma once
#include "kernels.h"

namespace mi {

struct AdapterPart {
  const float* a = nullptr;    // [K][rank]; null: the adapter does not cover this part
  const float* b = nullptr;    // [rank][n of the part]
  int rank = 0;
  float scale = 0.f;
  const float* gain = nullptr; // [n of the part] float32, DoRA; null: a plain LoRA entry
};

constexpr int LORA_ROWS_T_LD = 3 * 64;     // floats of t per token row: [part][64]
constexpr int LORA_ENGINE_COL = MI_MAX_ADAPTERS;       // the engine-wide adapter's column, behind the public slots
constexpr int LORA_TABLE_COLS = MI_MAX_ADAPTERS + 1;   // columns (adapters) of a table row

struct LoraRowsCall {
  const AdapterPart* table = nullptr;      // device [n_parts][LORA_TABLE_COLS]
  const int32_t* row_adapter = nullptr;    // device [M]: table column of every token row, -1 = none
  int n_parts = 0;
  int row0[3] = {0, 0, 0}, n[3] = {0, 0, 0};   // output columns [row0, row0 + n) of every part
  int M = 0, K = 0;
  int act = MI_F32, rnd = RND_NONE;
  float* t = nullptr;                      // device [M][LORA_ROWS_T_LD]
  bool gain = false;                       // some entry of the table carries a gain: the up-add's gain-aware instantiation
};

// x [M][ldx] in the activation dtype; pro / norm_w / eps: the linear's prologue.  K <= 36864.
int launch_lora_down_by_row(const LoraRowsCall& c, const void* x, int ldx, int pro, const void* norm_w, float eps,
                            hipStream_t st);
// y [M][ldy]: the stored output of the base linear.  resid != null ([M][ldr], one part whose row0 is 0): every row, adapted
// or not, ends with resid = R(resid + y'); y itself is then left as the linear stored it.
int launch_lora_up_add_by_row(const LoraRowsCall& c, void* y, int ldy, void* resid, int ldr, hipStream_t st);

// DoRA's gain of rows [row0, row0 + n) of a dense 16-bit matrix (W.wk = WK_BF16 / WK_F16, either layout, no quantisation):
//   gain[i] = m[i] / || W[row0 + i, :] + scale sum_j B[j][i] A[:, j] ||_2     (0 or NaN where the norm is 0: the caller checks)
// A [K][rank], B [rank][n], m [n], gain [n]: device float32.  float32 accumulation in a fixed order (lora_rows.hip), no atomics:
// the same inputs give the same bits, in both layouts.
int launch_dora_gain(const LinearW& W, int row0, int n, const float* A, const float* B, const float* m, int rank, float scale,
                     float* gain, hipStream_t st);

}  // namespace mi
