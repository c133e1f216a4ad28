"""GPU tests of the gim_lightglue pair-list path: KeypointBank (gim_lg_bank_put), LightGlue.match_pairs (gim_lg_gather_pairs) and the hloc
wire format (gim_lg_emit_hloc) against LightGlue.forward() on the same images stacked by hand.

The bar is EXACT equality throughout: match_pairs runs forward()'s own kernels behind its first block, so its outputs are forward()'s
bit for bit as soon as the gathered rows (X32, CAT[:, :256], enc) are -- and those must be, because the bank stores the same fp32
keypoints / sizes / descriptors (or, with fp16 storage, descriptors that forward() is given rounded to fp16) and converts with the same
instructions.

K = 72 keypoints: not a multiple of 64 (the SDPA padding path runs) and above 64 (two key tiles).  Seeded random weights."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lightglue_oracle as O

pytestmark = pytest.mark.gpu
K = 72
SIZES = [(640.0, 480.0), (500.0, 480.0), (320.0, 256.0), (1024.0, 768.0), (96.0, 128.0)]   # image_size (w, h): all different
PAIRS = [(0, 1), (0, 2), (1, 2), (2, 0), (1, 1)]   # a repeated image within a batch, a reversed pair, a self pair; batches of 4 -> 4 + 1
PRECISIONS = ["fp32", "bf16", "fp16"]
EXACT = ("matches0", "matches1", "matching_scores0", "matching_scores1", "ref_descriptors0", "ref_descriptors1")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _images():
    """5 images of K keypoints (CPU, never modified): views of one scene -- a permutation of shared points with jitter and descriptor noise
    -- so that the random-weight matcher has mutual matches to report"""
    g = torch.Generator().manual_seed(1234)
    base_xy = torch.rand(K, 2, generator=g)
    base_d = F.normalize(torch.randn(K, 256, generator=g), dim=-1)
    out = []
    for w, h in SIZES:
        perm = torch.randperm(K, generator=g)
        kp = (base_xy[perm] * torch.tensor([w - 1, h - 1]) + 0.3 * torch.randn(K, 2, generator=g)).clamp_(min=0)
        de = F.normalize(base_d[perm] + 0.03 * torch.randn(K, 256, generator=g), dim=-1)
        out.append((kp.contiguous(), de.contiguous(), torch.tensor([w, h])))
    return tuple(out)


def _model(precision, seed=0):
    from gim_amd.lightglue import LightGlue
    lg = LightGlue({"filter_threshold": 0.1, "flash": False, "checkpointed": True, "precision": precision})
    lg.load_state_dict(O.make_state_dicts(seed)[1])
    return lg.eval()


def _bank(storage, images=(0, 1, 2), slots=4):
    from gim_amd.lightglue import KeypointBank
    bank = KeypointBank(slots, K, storage=storage, device=_dev())
    for i in images:
        kp, de, sz = _images()[i]
        bank.put(i, kp.to(_dev()), de.to(_dev()), sz)
    return bank


def _stacked(pairs, half=False):
    """forward()'s input for `pairs`, stacked by hand; half: descriptors rounded to fp16 and cast back (what an fp16 bank holds)"""
    dev = _dev()
    data = {}
    for side in (0, 1):
        im = [_images()[p[side]] for p in pairs]
        de = torch.stack([x[1] for x in im])
        data[f"keypoints{side}"] = torch.stack([x[0] for x in im]).to(dev)
        data[f"descriptors{side}"] = (de.half().float() if half else de).to(dev)
        data[f"image_size{side}"] = torch.stack([x[2] for x in im]).to(dev)
    return data


def _capture(model):
    got = []
    model.input_hook = lambda X32, CAT, enc: got.append((X32.clone(), CAT[:, :256].clone(), enc.clone()))
    return got


def _assert_same(pred, ref, what):
    for k in EXACT:
        assert pred[k].dtype == ref[k].dtype and torch.equal(pred[k], ref[k]), f"{what}: {k} differs from forward()"
    assert len(pred["matches"]) == len(ref["matches"])
    for b in range(len(ref["matches"])):
        assert torch.equal(pred["matches"][b], ref["matches"][b]) and torch.equal(pred["scores"][b], ref["scores"][b]), (what, b)
    assert pred["stop"] == ref["stop"]


def _check_pair_list(model, bank, half, what):
    from gim_amd.lightglue.pairs import pair_batches
    got = _capture(model)
    batches = pair_batches(PAIRS, 4)
    assert [len(b) for b in batches] == [4, 1]
    matched = 0
    for batch in batches:
        del got[:]
        pred = model.match_pairs(bank, bank.slots([p[0] for p in batch]), bank.slots([p[1] for p in batch]))
        ref = model(_stacked(batch, half))
        assert len(got) == 2
        for name, a, b in zip(("X32", "CAT[:, :256]", "enc"), got[0], got[1]):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"{what}: gathered {name} differs from forward()'s"
        _assert_same(pred, ref, what)
        matched += int((ref["matches0"] > -1).sum())
    model.input_hook = None
    assert matched > 0, "the test inputs must produce matches"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fp32_bank_is_forward_bit_for_bit(precision):
    _check_pair_list(_model(precision), _bank("fp32"), False, f"fp32 bank, {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fp16_bank_is_forward_on_fp16_rounded_descriptors(precision):
    bank = _bank("fp16")
    assert bank.kpts.dtype == torch.float32 and bank.desc.dtype == torch.float16   # keypoints stay fp32 in the bank
    for i in range(3):
        s = bank.slots([i])[0]
        assert torch.equal(bank.kpts[s].cpu(), _images()[i][0]) and torch.equal(bank.desc[s].cpu(), _images()[i][1].half())
    _check_pair_list(_model(precision), bank, True, f"fp16 bank, {precision}")


class _Group(dict):
    """h5py's group protocol over a dict (`in` and `del` are dict's own)"""

    def create_group(self, name):
        self[name] = g = _Group()
        return g

    def create_dataset(self, name, data):
        self[name] = np.asarray(data)


def test_hloc_wire_format():
    from gim_amd import hloc_formats
    from gim_amd.lightglue import match_pair_list
    model, bank = _model("fp32"), _bank("fp32")
    batch = PAIRS[:4]
    pred = model.match_pairs(bank, bank.slots([p[0] for p in batch]), bank.slots([p[1] for p in batch]), hloc=True)
    assert pred["matches0_i16"].dtype == torch.int16 and pred["matching_scores0_f16"].dtype == torch.float16
    assert torch.equal(pred["matches0_i16"], pred["matches0"].short())
    assert torch.equal(pred["matching_scores0_f16"], pred["matching_scores0"].half())
    assert (pred["matches0"] > -1).any()
    # the whole list through the writer == the host writer given forward()'s results, pair by pair
    got, want = _Group(), _Group()
    out = match_pair_list(model, bank, PAIRS, batch_pairs=4, writer=got)
    assert [(a, b) for a, b, _, _ in out] == PAIRS
    for a, b in PAIRS:
        ref = model(_stacked([(a, b)]))
        hloc_formats.write_sparse_matches(want, str(a), str(b), ref["matches0"][0].cpu().numpy(), ref["matching_scores0"][0].cpu().numpy())
    assert list(got) == list(want) == [hloc_formats.pair_key(str(a), str(b)) for a, b in PAIRS]
    for key in want:
        assert set(got[key]) == {"matches0", "matching_scores0"}
        for ds in ("matches0", "matching_scores0"):
            assert got[key][ds].dtype == want[key][ds].dtype and np.array_equal(got[key][ds], want[key][ds]), (key, ds)


def test_hloc_emit_tail_and_range():
    """a count that is no multiple of the 8 elements a lane converts, scores on both sides of fp16's rounding, and the int16 bound"""
    from gim_amd import ops
    from gim_amd._lib import GimHipError
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    r = ops.AssignResult()
    r.matches0 = torch.randint(-1, 32767, (3, 37), generator=g).to(dev)
    r.matches0[0, :3] = torch.tensor([-1, 32766, 0], device=dev)
    r.mscores0 = torch.rand(3, 37, generator=g).to(dev)
    r.mscores0[0, :4] = torch.tensor([0.0, 1.0, 1e-8, 0.33337], device=dev)
    m, s = ops.lg_emit_hloc(r)
    assert torch.equal(m, r.matches0.short()) and torch.equal(s, r.mscores0.half())
    r.matches0 = torch.zeros(1, 32768, dtype=torch.int64, device=dev)
    r.mscores0 = torch.zeros(1, 32768, device=dev)
    with pytest.raises(GimHipError, match="32767"):
        ops.lg_emit_hloc(r)


def test_lru_eviction():
    from gim_amd._lib import GimHipError
    model = _model("fp32")
    bank = _bank("fp32", images=(0, 1, 2, 3))
    bank.slots([0])                               # image 0 is used: image 1 is now the least recently used
    kp, de, sz = _images()[4]
    slot4 = bank.put(4, kp.to(_dev()), de.to(_dev()), sz)
    assert 1 not in bank and all(i in bank for i in (0, 2, 3, 4)) and bank.stats.evictions == 1
    pred = model.match_pairs(bank, bank.slots([4, 0]), bank.slots([0, 4]))
    _assert_same(pred, model(_stacked([(4, 0), (0, 4)])), "after eviction")
    assert bank.slots([4]) == [slot4]
    with pytest.raises(GimHipError, match="not resident"):   # image 1's old slot holds image 4 now: never read it for image 1
        bank.slots([1, 2])
    with pytest.raises(GimHipError, match="not resident"):
        from gim_amd.lightglue import match_pair_list
        match_pair_list(model, bank, [(0, 2), (1, 2)], batch_pairs=4)


def test_encodings_follow_the_module():
    model, bank = _model("fp32"), _bank("fp32")
    batch = PAIRS[:4]
    s0, s1 = bank.slots([p[0] for p in batch]), bank.slots([p[1] for p in batch])
    _assert_same(model.match_pairs(bank, s0, s1), model(_stacked(batch)), "first weights")
    enc_old = bank.enc.clone()
    model.load_state_dict(O.make_state_dicts(7)[1])           # another posenc.Wr: the table in the bank is stale
    got = _capture(model)
    pred = model.match_pairs(bank, s0, s1)
    ref = model(_stacked(batch))
    assert torch.equal(got[0][2], got[1][2]), "encodings were not rebuilt from the new Wr"
    _assert_same(pred, ref, "after load_state_dict")
    used = sorted(set(s0 + s1))
    assert not torch.equal(bank.enc[used], enc_old[used])
    # images inserted after the rebuild get the new module's encodings in the insertion launch itself; another module takes the bank over
    kp, de, sz = _images()[3]
    bank.put(3, kp.to(_dev()), de.to(_dev()), sz)
    _assert_same(model.match_pairs(bank, bank.slots([3]), bank.slots([0])), model(_stacked([(3, 0)])), "inserted after the rebuild")
    other = _model("fp32", seed=11)
    _assert_same(other.match_pairs(bank, bank.slots([3]), bank.slots([0])), other(_stacked([(3, 0)])), "second module")
