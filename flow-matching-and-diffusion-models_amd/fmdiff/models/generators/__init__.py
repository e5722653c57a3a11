from .diffusionfactory import DiffusionUNetFactory
from .vaefactory import VAEFactory

__all__ = ["DiffusionUNetFactory", "VAEFactory"]
