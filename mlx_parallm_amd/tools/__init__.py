"""Command-line tools of the package (the reference's ``mlx_parallm/tools``)."""
