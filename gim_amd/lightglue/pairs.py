"""The SfM shape of gim_lightglue (reconstruction.py `--version gim_lightglue`: SuperPoint once per image, LightGlue over an exhaustive
pair list, hloc/match_features.py:124-160, 244-255): the detector runs once per IMAGE into a `KeypointBank`, the matcher takes the
pairs by slot index from the bank, `batch_pairs` pairs per launch sequence.

  extract_to_bank(detector, images, bank, keys)        n detector calls and n insertions for n images
  match_pair_list(model, bank, pairs, batch_pairs=8)   every pair it is given, in the order given, cut into batches (a short last one
                                                       is allowed).  It orders nothing and dedups nothing: dropping (j, i) when (i, j)
                                                       is listed is hloc's find_unique_new_pairs (match_features.py:192-210), on the
                                                       caller's side.

Results go to `writer`, any object with h5py's group protocol (`in`, `del`, `create_group`, `create_dataset`: an `h5py.File` where it is
installed -- h5py is not a dependency), as gim_amd.hloc_formats.write_sparse_matches lays them out: one group per pair with `matches0`
int16 and `matching_scores0` fp16.  The two datasets leave the device already in that format (gim_lg_emit_hloc), one copy per batch.
"""
import torch

from .._lib import GimHipError
from ..bank import pair_batches, sparse_pair_list  # noqa: F401  (pair_batches: re-exported)


@torch.no_grad()
def extract_to_bank(detector, images, bank, keys=None, image_sizes=None, model=None):
    """Runs `detector` (gim_amd.lightglue.SuperPoint with max_num_keypoints <= bank.num_keypoints; with force_num_keypoints every image
    fills its slot, padded with random keypoints as the reference pads, without it the bank stores what the detector found) ONCE per
    image and inserts the result under keys[i] (default: i).  images: a sequence of [1|3, H, W] or [1, 1|3, H, W] device tensors (sizes
    may differ).  image_sizes[i]: what the matcher is to get as the image's `image_size` ((w, h)); default: the tensor's own.
    model: the LightGlue module that will match -- with it the encodings are written by the insertions themselves.
    Returns the keys."""
    images = list(images)
    keys = list(range(len(images))) if keys is None else list(keys)
    if len(keys) != len(images):
        raise ValueError(f"{len(images)} images, {len(keys)} keys")
    if model is not None:
        bank.bind(model)
    for i, (key, img) in enumerate(zip(keys, images)):
        img = img[None] if img.dim() == 3 else img
        out = detector({"image": img.to(bank.device)})
        if out["keypoints"].shape[1] > bank.num_keypoints:
            raise GimHipError(f"the detector returned {out['keypoints'].shape[1]} keypoints for image {key!r}, the bank holds at most "
                              f"{bank.num_keypoints} per image: set max_num_keypoints")
        size = image_sizes[i] if image_sizes is not None else (img.shape[-1], img.shape[-2])
        bank.put(key, out["keypoints"][0], out["descriptors"][0], torch.as_tensor(size))
    return keys


@torch.no_grad()
def match_pair_list(model, bank, pairs, batch_pairs=8, writer=None, names=None):
    """pairs: a sequence of (key0, key1) of images resident in `bank`.  Returns [(key0, key1, matches0 int16 [n0], matching_scores0 fp16
    [n0])] as numpy arrays, n0 = the keypoint count of image key0, in the order of `pairs`; with `writer` every pair is also written as
    hloc stores it (group name from names[key] if `names` is given, else str(key))."""
    def match_batch(s0, s1):
        pred = model.match_pairs(bank, s0, s1, hloc=True)
        return zip(pred["matches0_i16"].cpu().numpy(), pred["matching_scores0_f16"].cpu().numpy())
    return sparse_pair_list(bank, pairs, batch_pairs, match_batch, writer, names, counts0=getattr(bank, "slot_counts", None))
