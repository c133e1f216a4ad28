"""GPU tests of ragged keypoint counts in the gim_lightglue bank / pair-list path.  The contract: pair p of a ragged batch gets what
forward() gives for that pair alone with its own (n0, n1) keypoints.

Bank capacity K = 200 (no multiple of 64 or 128), six images with counts {200, 129, 64, 63, 5, 0}, match-rich planted descriptors,
seeded weights.  BOUND: the largest difference of matching_scores0/1 that forward() on the parent commit shows between a pair at B = 1
and the same pair inside a B = 2 call is 0 in fp32, bf16 and fp16 (measured on the parent's own build for the pairs (0, 1) and (1, 3) of
this file at their own sizes) -- so a pair's valid outputs must be bit-equal to forward() at B = 1, whatever batch it rides in."""
import functools

import numpy as np
import pytest
import torch

import lightglue_oracle as O

pytestmark = pytest.mark.gpu
K = 200
COUNTS = [200, 129, 64, 63, 5, 0]
SIZES = [(640.0, 480.0), (500.0, 480.0), (320.0, 256.0), (640.0, 480.0), (96.0, 128.0), (64.0, 64.0)]
PAIRS = [(0, 1), (1, 0), (1, 3), (2, 1), (4, 0), (0, 0)]          # repeated and swapped images, a tiny image, a self pair
PAIRS_EMPTY = [(5, 1), (1, 5), (0, 1)]                            # an image without keypoints, on either side
PRECISIONS = ["fp32", "bf16", "fp16"]
AGREE = {"fp32": 1.0, "bf16": 0.985, "fp16": 0.99}                # the bars of test_gpu_lightglue.py::test_lightglue_unequal_counts_and_bf16
VALID = ("matches0", "matching_scores0", "matches1", "matching_scores1")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _images():
    """views of one planted scene (view A = image 0 of the planted pair, view B = image 1): image i keeps the first COUNTS[i] keypoints
    of its view -- B rolled by 80 for image 2 -- so every pair of PAIRS shares many correspondences"""
    kp0, d0, kp1, d1 = O.planted_descriptors(1, K, seed=17)
    A, Bv = (kp0[0], d0[0]), (kp1[0], d1[0])
    views = [A, Bv, (Bv[0].roll(-80, 0), Bv[1].roll(-80, 0)), Bv, A, A]
    return tuple((kp[:n].contiguous(), de[:n].contiguous(), torch.tensor(sz)) for (kp, de), n, sz in zip(views, COUNTS, SIZES))


@functools.lru_cache(maxsize=None)
def _model(precision):
    from gim_amd.lightglue import LightGlue
    lg = LightGlue({"filter_threshold": 0.1, "flash": False, "checkpointed": True, "precision": precision})
    lg.load_state_dict(O.make_state_dicts(0)[1])
    return lg.eval()


def _bank(capacity=K, images=range(6), slots=6, pad_to=None):
    from gim_amd.lightglue import KeypointBank
    bank = KeypointBank(slots, capacity, storage="fp32", device=_dev())
    for t in (bank.kpts, bank.desc, bank.enc):
        t.fill_(float("nan"))
    for i in images:
        kp, de, sz = _images()[i]
        bank.put(i, kp.to(_dev()), de.to(_dev()), sz)
    return bank


def _pair_data(a, b):
    (k0, d0, s0), (k1, d1, s1) = _images()[a], _images()[b]
    return {"keypoints0": k0[None], "descriptors0": d0[None], "image_size0": s0[None],
            "keypoints1": k1[None], "descriptors1": d1[None], "image_size1": s1[None]}


@functools.lru_cache(maxsize=None)
def _single(precision, a, b):
    """forward() at B = 1 on the pair's own keypoints (computed once per pair, left unchanged)"""
    pred = _model(precision)({k: v.to(_dev()) for k, v in _pair_data(a, b).items()})
    return {k: pred[k][0].clone() for k in VALID} | {"matches": pred["matches"][0].clone(), "scores": pred["scores"][0].clone()}


@functools.lru_cache(maxsize=None)
def _oracle(a, b):
    return O.lightglue_forward(O.make_state_dicts(0)[1], _pair_data(a, b))["matches0"][0]


def _match(precision, bank, pairs, **kw):
    return _model(precision).match_pairs(bank, bank.slots([p[0] for p in pairs]), bank.slots([p[1] for p in pairs]), **kw)


def _assert_pair(pred, i, ref, n0, n1, what):
    for key, n in (("matches0", n0), ("matching_scores0", n0), ("matches1", n1), ("matching_scores1", n1)):
        assert torch.equal(pred[key][i, :n], ref[key]), f"{what}: {key} differs from forward() on the pair alone"
        pad = pred[key][i, n:]
        assert bool((pad == -1).all()) if key.startswith("matches") else not pad.any(), f"{what}: {key} behind the length"
    assert torch.equal(pred["matches"][i], ref["matches"]) and torch.equal(pred["scores"][i], ref["scores"]), f"{what}: match list"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_counts_through_the_ragged_entry(precision):
    """every image fills its slot: the ragged kernels, forced on, give today's match_pairs bit for bit"""
    from gim_amd.lightglue import KeypointBank
    bank = KeypointBank(3, K, storage="fp32", device=_dev())
    kp0, d0, kp1, d1 = O.planted_descriptors(1, K, seed=17)
    for i, (kp, de) in enumerate(((kp0[0], d0[0]), (kp1[0], d1[0]), (kp0[0].flip(0), d0[0].flip(0)))):
        bank.put(i, kp.to(_dev()), de.to(_dev()), torch.tensor(SIZES[i]))
    pairs = [(0, 1), (1, 2), (2, 0), (1, 1)]
    uni, rag = _match(precision, bank, pairs), _match(precision, bank, pairs, ragged=True)
    assert "num_keypoints0" not in uni and rag["num_keypoints0"].tolist() == [K] * 4 == rag["num_keypoints1"].tolist()
    for key in VALID + ("ref_descriptors0", "ref_descriptors1", "prune0", "prune1"):
        assert torch.equal(uni[key], rag[key]), key
    for b in range(len(pairs)):
        assert torch.equal(uni["matches"][b], rag["matches"][b]) and torch.equal(uni["scores"][b], rag["scores"][b])
    assert sum(len(m) for m in uni["matches"]) > 50


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_bank_is_forward_per_pair(precision):
    bank = _bank()
    pred = _match(precision, bank, PAIRS)
    assert pred["num_keypoints0"].tolist() == [COUNTS[a] for a, _ in PAIRS] and pred["num_keypoints1"].tolist() == [COUNTS[b] for _, b in PAIRS]
    assert pred["matches0"].shape == (len(PAIRS), K) and pred["matches0"].dtype == torch.int64
    for i, (a, b) in enumerate(PAIRS):
        _assert_pair(pred, i, _single(precision, a, b), COUNTS[a], COUNTS[b], f"{precision} pair {(a, b)}")
        want = _oracle(a, b)
        found = int((want > -1).sum())
        assert found > min(COUNTS[a], COUNTS[b]) / 4, f"the oracle finds {found} matches on pair {(a, b)}: the inputs are not match-rich"
        agree = (pred["matches0"][i, :COUNTS[a]].cpu() == want).float().mean().item()
        print(f"[agree] ragged lightglue {precision} pair {(a, b)}: matches0 agreement with the fp32 oracle {agree:.4f}")
        assert agree >= AGREE[precision], (precision, (a, b), agree)


def test_an_image_without_keypoints():
    bank = _bank()
    pred = _match("fp32", bank, PAIRS_EMPTY)
    for i in (0, 1):
        assert (pred["matches0"][i] == -1).all() and (pred["matches1"][i] == -1).all() and len(pred["matches"][i]) == 0
        assert not pred["matching_scores0"][i].any() and not pred["matching_scores1"][i].any()
    _assert_pair(pred, 2, _single("fp32", 0, 1), COUNTS[0], COUNTS[1], "next to empty pairs")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_padding_and_batch_independent(precision):
    """the same list from a bank of capacity 264, and every pair at B = 1 from the bank: the same valid outputs bit for bit"""
    wide = _match(precision, _bank(capacity=264), PAIRS)
    bank = _bank()
    for i, (a, b) in enumerate(PAIRS):
        ref = _single(precision, a, b)
        _assert_pair(wide, i, ref, COUNTS[a], COUNTS[b], f"{precision} capacity 264, pair {(a, b)}")
        _assert_pair(_match(precision, bank, [(a, b)], ragged=True), 0, ref, COUNTS[a], COUNTS[b], f"{precision} B = 1, pair {(a, b)}")


def test_forward_with_lengths_equals_the_bank_path():
    dev = _dev()
    bank = _bank()
    want = _match("fp32", bank, PAIRS)
    data = {}
    for side in (0, 1):
        kp = torch.full((len(PAIRS), K, 2), 3.0)
        de = torch.full((len(PAIRS), K, 256), float("nan"))       # what a caller leaves in the padding is not read into a result
        for i, p in enumerate(PAIRS):
            k, d, _ = _images()[p[side]]
            kp[i, :len(k)], de[i, :len(k)] = k, d
        data[f"keypoints{side}"], data[f"descriptors{side}"] = kp.to(dev), de.to(dev)
        data[f"image_size{side}"] = torch.stack([_images()[p[side]][2] for p in PAIRS]).to(dev)
        data[f"num_keypoints{side}"] = torch.tensor([COUNTS[p[side]] for p in PAIRS])
    got = _model("fp32")(data)
    for key in VALID:
        assert torch.equal(got[key], want[key]), key
    for b in range(len(PAIRS)):
        assert torch.equal(got["matches"][b], want["matches"][b]) and torch.equal(got["scores"][b], want["scores"][b])
    assert got["num_keypoints0"].tolist() == want["num_keypoints0"].tolist()
    # absent keys: today's behaviour
    plain = _model("fp32")({k: v.to(dev) for k, v in _pair_data(0, 1).items()})
    assert "num_keypoints0" not in plain and plain["matches1"].shape == (1, COUNTS[1])


class _Group(dict):
    def create_group(self, name):
        self[name] = g = _Group()
        return g

    def create_dataset(self, name, data):
        self[name] = np.asarray(data)


def test_pair_list_writes_rows_of_image0s_length():
    from gim_amd import hloc_formats
    from gim_amd.lightglue import match_pair_list
    bank, w = _bank(), _Group()
    pairs = PAIRS + PAIRS_EMPTY
    out = match_pair_list(_model("fp32"), bank, pairs, batch_pairs=4, writer=w)
    assert [(a, b) for a, b, _, _ in out] == pairs
    for (a, b), (_, _, m, s) in zip(pairs, out):
        assert m.dtype == np.int16 and s.dtype == np.float16 and m.shape == s.shape == (COUNTS[a],)
        pred = _match("fp32", bank, [(a, b)], ragged=True)
        assert np.array_equal(m, pred["matches0"][0, :COUNTS[a]].short().cpu().numpy())
        assert np.array_equal(s, pred["matching_scores0"][0, :COUNTS[a]].half().cpu().numpy())
        g = w[hloc_formats.pair_key(str(a), str(b))]
        assert np.array_equal(g["matches0"], m) and np.array_equal(g["matching_scores0"], s)


def test_plugin_reads_features_with_varying_counts():
    from gim_amd import hloc_formats
    from gim_amd.hloc_matchers.gim_lightglue_hip import GimLightGlueHip
    plug = GimLightGlueHip({"precision": "fp32", "storage": "fp32", "batch_pairs": 4})
    plug.net.load_state_dict(O.make_state_dicts(0)[1])
    feats = {str(i): {"keypoints": kp.numpy(), "descriptors": de.t().contiguous().numpy(), "image_size": sz.numpy()}
             for i, (kp, de, sz) in enumerate(_images())}
    pairs = [(str(a), str(b)) for a, b in PAIRS + PAIRS_EMPTY]
    w = _Group()
    out = plug.match_pairs_from_features(feats, pairs, w, device=_dev())
    for (a, b, m, s), (ia, ib) in zip(out, PAIRS + PAIRS_EMPTY):
        assert m.shape == (COUNTS[ia],) and set(w[hloc_formats.pair_key(a, b)]) == {"matches0", "matching_scores0"}
        if COUNTS[ia] and COUNTS[ib]:
            assert np.array_equal(m, _single("fp32", ia, ib)["matches0"].short().cpu().numpy()), (a, b)


def test_extract_to_bank_stores_what_the_detector_found():
    from gim_amd.lightglue import KeypointBank, SuperPoint, extract_to_bank
    sp_sd = O.make_state_dicts(0)[0]
    img = O.seeded_gray(1, 64, 64, 7)[0] * 0.02 + 0.5           # flat-ish
    img[:, 20:28, 20:28] += 0.4
    # a threshold that only the 30 best pixels of the oracle's score map pass: at most 30 detections whatever the seeded weights do
    thr = float(O.superpoint_dense(sp_sd, img[None])[0][0, 4:-4, 4:-4].flatten().topk(31).values[-1])
    det = SuperPoint({"max_num_keypoints": 64, "force_num_keypoints": False, "detection_threshold": thr, "nms_radius": 3,
                      "trainable": False, "precision": "fp32"})
    det.load_state_dict(sp_sd)
    det = det.eval()
    ref = det({"image": img[None].to(_dev())})
    n = ref["keypoints"].shape[1]
    assert 0 < n < 64, f"the test image must yield some, but fewer than 64 keypoints, got {n}"
    bank = KeypointBank(2, 64, storage="fp32", device=_dev())
    extract_to_bank(det, [img], bank, keys=["im"])
    s = bank.slots(["im"])[0]
    assert bank.counts[s] == n and int(bank.n[s]) == n
    assert torch.equal(bank.kpts[s, :n], ref["keypoints"][0]) and torch.equal(bank.desc[s, :n], ref["descriptors"][0])
    assert not bank.kpts[s, n:].any() and not bank.desc[s, n:].any()       # no random padding is stored


def test_errors_come_before_any_launch():
    from gim_amd._lib import GimHipError
    bank = _bank(images=(0, 1), slots=2)
    before = (bank.kpts.clone(), list(bank.counts), bank.table.keys())
    with pytest.raises(GimHipError, match="holds 200"):
        bank.put(9, torch.zeros(201, 2, device=_dev()), torch.zeros(201, 256, device=_dev()), torch.tensor([64.0, 48.0]))
    assert 9 not in bank and list(bank.counts) == before[1] and bank.table.keys() == before[2]
    assert torch.equal(torch.nan_to_num(bank.kpts), torch.nan_to_num(before[0]))
    kp, de, sz = _images()[2]
    bank.put(2, kp.to(_dev()), de.to(_dev()), sz)                # evicts image 0
    from gim_amd.lightglue import match_pair_list
    with pytest.raises(GimHipError, match="not resident"):
        match_pair_list(_model("fp32"), bank, [(1, 2), (0, 1)], batch_pairs=4)
