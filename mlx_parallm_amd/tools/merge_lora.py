"""``python -m mlx_parallm_amd.tools.merge_lora --base-model <dir> --lora-path <dir> --output-path <dir> [--de-quantize]``

Writes a checkpoint directory whose weights have the adapter merged in (``merge.merge_adapter_into_weights``, on the device)
and that ``utils.load`` reads with no adapter: safetensors, ``config.json`` and the tokenizer files copied over.  The flag names
are those of the reference's stub (``mlx_parallm/tools/merge_lora.py``: "full merge is non-trivial and will be implemented
later").  A quantised base comes out re-quantised with its own bits and group.  ``--de-quantize`` merges into the dequantised
matrices instead, dequantises every other quantised tensor through ``convert.dequantize_model`` and drops ``quantization`` from
the config, as mlx-lm's ``fuse`` does -- which also keeps the parts of a fused q|k|v from mixing dense and packed weights.
"""
from __future__ import annotations

import argparse
import glob
import shutil
from pathlib import Path
from typing import Optional, Sequence

TOKENIZER_FILES = ("tokenizer*", "special_tokens_map.json", "vocab.*", "merges.txt", "added_tokens.json", "chat_template*",
                   "generation_config.json")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="mlx_parallm_amd.tools.merge_lora", description="Merge a LoRA / DoRA adapter into a base model")
    p.add_argument("--base-model", required=True, help="Directory of the base model.")
    p.add_argument("--lora-path", required=True, help="Adapter directory (adapter_config.json + adapters.safetensors).")
    p.add_argument("--output-path", required=True, help="Directory to write the merged model to.")
    p.add_argument("--de-quantize", action="store_true", help="Write a dense model from a quantised base.")
    p.add_argument("--device", type=int, default=0, help="HIP device index the merge kernels run on.")
    return p


def merge(base_model: str, lora_path: str, output_path: str, de_quantize: bool = False, device: int = 0) -> Path:
    """-> the directory written.  ``ValueError``: the output is the base or the adapter directory, or it exists and is not
    empty, or ``de_quantize`` on a base that is not quantised; everything ``merge_adapter_into_weights`` raises."""
    from ..convert import dequantize_model, load_weights_dir, save_config, save_weights
    from ..merge import merge_adapter_into_weights
    from ..utils import get_model_path, load_config

    model_path = get_model_path(base_model)
    out = Path(output_path)
    if out.resolve() in (model_path.resolve(), Path(lora_path).resolve()):
        raise ValueError(f"--output-path {out} is the base model or the adapter directory: nothing is merged in place")
    if out.exists() and (not out.is_dir() or any(out.iterdir())):
        raise ValueError(f"--output-path {out} exists and is not an empty directory")
    config = load_config(model_path)
    if de_quantize and not config.get("quantization"):
        raise ValueError("--de-quantize: the base model is not quantised")
    weights = load_weights_dir(model_path)
    merged = merge_adapter_into_weights(weights, config, lora_path, device=device, de_quantize=de_quantize)
    if de_quantize:
        weights, config = dequantize_model(weights, config)
    save_weights(out, weights, donate_weights=True)
    for pat in TOKENIZER_FILES:
        for f in glob.glob(str(model_path / pat)):
            shutil.copy(f, out)
    save_config(config, config_path=out / "config.json")
    print(f"[INFO] merged {len(merged)} projections of {lora_path} into {out}")
    return out


def main(argv: Optional[Sequence[str]] = None) -> int:
    parser = build_parser()
    ns = parser.parse_args(argv)
    try:
        merge(ns.base_model, ns.lora_path, ns.output_path, de_quantize=ns.de_quantize, device=ns.device)
    except ValueError as e:
        parser.error(str(e))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
