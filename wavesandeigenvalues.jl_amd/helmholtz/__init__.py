"""Producers of LinearOperatorFamily objects for the device hot path (the slot Helmholtz.discretize fills)."""
from . import annulus  # noqa: F401
from .family import annulus_family, helmholtz_family, speaker_source  # noqa: F401
from .refine import RefinedMesh, octosplit  # noqa: F401
from .locate import Locator  # noqa: F401
