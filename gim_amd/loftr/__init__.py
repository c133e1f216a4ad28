from .config import get_cfg_defaults, lower_config  # noqa: F401
from .loftr import LoFTR, LoFTRFeatures, StaleFeaturesError  # noqa: F401
from .bank import CachedPairMatcher, FeatureBank  # noqa: F401
