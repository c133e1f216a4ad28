from .superpoint import SuperPoint  # noqa: F401
from .lightglue import LightGlue  # noqa: F401
from .pipeline import gim_lightglue_inference  # noqa: F401
from .bank import KeypointBank  # noqa: F401
from .pairs import extract_to_bank, match_pair_list  # noqa: F401
