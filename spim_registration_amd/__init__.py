"""spim_registration_amd: the SPIM registration / deconvolution stages on MI355X."""
from . import dom  # noqa: F401  (the Difference-of-Mean detector, beside ``dog``)

__all__ = ["dom"]
