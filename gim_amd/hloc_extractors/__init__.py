"""Drop-in `hloc.extractors` plugins backed by the HIP engine.

hloc looks an extractor up with `dynamic_load(hloc.extractors, conf['model']['name'])` (`hloc/utils/base_model.py:36-47`), exactly as it
does a matcher: copy (or symlink) `gim_superpoint_hip.py` into the reference's `hloc/extractors/` -- or put this package on the path as
`hloc.extractors` -- and select it with `feature_conf['model']['name'] = 'gim_superpoint_hip'`.  The base class is hloc's own
`BaseModel` (gim_amd/hloc_matchers/base.py): without hloc on the path the plugin modules do not import.
"""
