"""jen1_amd: the JEN-1 denoiser path and its audio front and back ends on hand-written HIP for gfx950.  Submodules are imported on
first use (``jen1_amd.spectral`` and ``jen1_amd.effects`` among them), so importing the package loads nothing."""
import importlib

__all__ = ["spectral", "effects"]


def __getattr__(name):
    if name in __all__:
        return importlib.import_module("." + name, __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
