"""spim_registration_amd: the SPIM registration / deconvolution stages on MI355X."""
from . import boundingbox  # noqa: F401  (the bounding box estimated from the data)
from . import dom  # noqa: F401  (the Difference-of-Mean detector, beside ``dog``)

__all__ = ["boundingbox", "dom"]
