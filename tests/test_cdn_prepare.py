"""prepare_for_cdn without a GPU (uvhand_amd/utils/denoising.py, csrc/msda_cdn.hip): the composition route against the fixture
made by running the reference's function (tests/golden/gen_cdn_prepare.py) bit for bit, drawing cases and generator state
included; the C ABI of the new entries (exported, in the binding's table, argument errors as codes before any launch — the fake
device addresses below never reach a kernel); the restated draws; dn_post_process; the host arithmetic of the group count."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cdn_prepare_inputs as CI  # noqa: E402

from uvhand_amd.utils import (cdn_attention_mask, cdn_draws, cdn_group_arithmetic, dn_post_process, prepare_for_cdn,  # noqa: E402
                              prepare_for_cdn_composition)

P = 0x10000                      # 16-byte aligned fake device address, only passed next to an argument the checks refuse
ERR_ARGUMENT = 1
NEW_ENTRIES = ("msda_cdn_supported", "msda_cdn_prepare_forward_f32", "msda_cdn_prepare_backward_f32")


@pytest.fixture(scope="module")
def golden():
    return load_golden("cdn_prepare")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


# ---- the composition against the reference's own run ----------------------------------------------------------------------------
@pytest.mark.parametrize("fn", [prepare_for_cdn_composition, prepare_for_cdn], ids=["composition", "drop_in_on_cpu"])
@pytest.mark.parametrize("case", list(CI.CASES))
def test_composition_equals_the_reference_bit_for_bit(case, fn, golden):
    """On CPU tensors the drop-in takes the composition route, so both names must reproduce the reference: layout, labels,
    keys, mask, dn_meta, the weight gradient, and — in the drawing cases — the generator's state afterwards."""
    label, key, mask, meta, grad, nxt = CI.run(fn, case)
    assert np.array_equal(label.detach().numpy(), golden[case + "/label"])
    assert label.dtype == torch.float32 and key.dtype == torch.float32
    assert np.array_equal(key.numpy(), golden[case + "/key"])
    assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), golden[case + "/mask"])
    assert meta == {"pad_size": int(golden[case + "/meta"][0]), "num_dn_group": int(golden[case + "/meta"][1])}
    assert all(type(v) is int for v in meta.values())
    assert meta["num_dn_group"] == CI.EXPECTED_GROUPS[case]
    assert (grad is None) == (case + "/grad_weight" not in golden)
    if grad is not None:
        assert np.array_equal(grad.numpy(), golden[case + "/grad_weight"])
    if nxt is not None:
        assert np.array_equal(nxt.numpy(), golden[case + "/next"])           # the generator's state after the call
        again = CI.run(fn, case)                                              # a second run of the same seed
        assert torch.equal(again[0], label) and torch.equal(again[5], nxt)


def test_drawing_cases_do_flip_labels(golden):
    """The fixture's ratio-0.5 cases are not the ratio-0 result by accident."""
    for case in ("flip_div33_h8", "flip_pair_h256"):
        c = dict(CI.CASES[case], ratio=0.0)
        enc, tg = CI.label_enc(case), CI.targets(case)
        plain = prepare_for_cdn_composition((tg, c["dn"], 0.0, c["box"]), True, CI.QUERIES, CI.NUM_CLASSES, c["hidden"], enc)[0]
        assert not np.array_equal(plain.detach().numpy(), golden[case + "/label"])


def test_box_noise_scale_is_dead_and_key_noise_is_not():
    """dn_components.py:104-105 are commented out: box_noise_scale changes nothing unless key_noise=True asks for the noise."""
    case = "flip_pair_h256"
    c, enc, tg = CI.CASES[case], CI.label_enc(case), CI.targets(case)
    outs = []
    for box, kn in ((0.0, False), (0.4, False), (0.4, True)):
        torch.manual_seed(7)
        outs.append(prepare_for_cdn_composition((tg, c["dn"], 0.0, box), True, CI.QUERIES, CI.NUM_CLASSES, c["hidden"], enc,
                                                key_noise=kn)[1])
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], outs[2])
    assert not bool(outs[2][0, 2::3].any()) and bool(outs[2][0, 0::3].any())         # frame 0 has 2 of single_pad = 3 targets


def test_labels_are_checked_on_the_host():
    case = "one_h8"
    enc, tg = CI.label_enc(case), CI.targets(case)
    with pytest.raises(IndexError, match="num_classes"):
        prepare_for_cdn((tg, 2, 0.5, 0.0), True, CI.QUERIES, CI.NUM_CLASSES + 2, 8, enc)
    for bad in (-1, CI.NUM_CLASSES + 1):
        with pytest.raises(IndexError, match="label"):
            prepare_for_cdn((dict(tg, labels=[[bad]]), 2, 0.0, 0.0), True, CI.QUERIES, CI.NUM_CLASSES, 8, enc)


def test_not_training_returns_four_nones():
    assert prepare_for_cdn(None, False, 5, 14, 8, None) == (None, None, None, None)
    assert prepare_for_cdn_composition(None, False, 5, 14, 8, None) == (None, None, None, None)


def test_composition_with_draws_is_the_restated_hash():
    """draws= replaces the generator: labels flip exactly where cdn_draws says, to the labels it says, and the generator is
    not touched."""
    case = "flip_div33_h8"
    c, enc, tg = CI.CASES[case], CI.label_enc(case), CI.targets(case)
    T, groups = sum(c["sizes"]), CI.EXPECTED_GROUPS[case]
    E = 2 * groups * T
    d = cdn_draws(1234567, E, CI.W, CI.NUM_CLASSES, c["ratio"], key_noise=True)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    label, key, _, meta = prepare_for_cdn_composition(CI.dn_args(case, tg), True, CI.QUERIES, CI.NUM_CLASSES, c["hidden"], enc,
                                                      key_noise=True, draws=d)
    assert torch.equal(torch.get_rng_state(), state)
    flat = torch.tensor([x for l in tg["labels"] for x in l]).repeat(2 * groups)
    want = torch.where(d.flip, d.new_label, flat)
    assert 0 < int(d.flip.sum()) < E
    single_pad, off = max(c["sizes"]), np.cumsum((0,) + c["sizes"])
    for b, n in enumerate(c["sizes"]):
        for r in range(2 * groups):
            for j in range(n):
                e = r * T + off[b] + j
                assert torch.equal(label[b, r * single_pad + j], enc.weight[want[e]])
    assert float(key.abs().max()) <= -math.log(1e-5 / (1 - 1e-5)) + 1e-3


# ---- the restated draws ------------------------------------------------------------------------------------------------------
def _scalar_hash(counter, seed):
    m = 0xFFFFFFFF
    mix = ((seed & m) + ((seed >> 32) & m) * 0x85EBCA6B) & m
    x = (counter + mix) & m
    x = ((x ^ (x >> 16)) * 0x85EBCA6B) & m
    return ((x ^ (x >> 13)) * 0xC2B2AE35) & m


def test_cdn_draws_is_the_counter_hash_and_deterministic_per_seed():
    seed, E, W, K = 0x1234567887654321, 37, 5, 14
    a = cdn_draws(seed, E, W, K, 0.5, key_noise=True)
    b = cdn_draws(torch.tensor([seed], dtype=torch.int64), E, W, K, 0.5, key_noise=True)
    other = cdn_draws(seed + 1, E, W, K, 0.5, key_noise=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a.new_label, other.new_label) and not torch.equal(a.magnitude, other.magnitude)
    thr = min(2 ** 32 - 1, int(0.5 * 0.5 * 2 ** 32))
    for e in (0, 1, 17, E - 1):                                   # element by element against Python integers
        assert bool(a.flip[e]) == (_scalar_hash(2 * e, seed) < thr)
        assert int(a.new_label[e]) == (_scalar_hash(2 * e + 1, seed) * K) >> 32
        for c in (0, W - 1):
            k = 2 * E + 2 * (e * W + c)
            assert float(a.sign[e, c]) == (1.0 if _scalar_hash(k, seed) >> 31 else -1.0)
            assert float(a.magnitude[e, c]) == (_scalar_hash(k + 1, seed) >> 8) * 2.0 ** -24
    assert a.sign.dtype == torch.float32 and a.magnitude.dtype == torch.float32 and a.new_label.dtype == torch.int64
    none = cdn_draws(seed, E, W, K, 0.0)
    assert not bool(none.flip.any()) and none.sign is None and none.magnitude is None


def test_flip_rate_and_new_labels():
    """E = 20 000 elements at ratio 0.5: a label flips with probability 0.25, so the count is binomial with standard deviation
    sqrt(E * 0.25 * 0.75) = 61.2; the bound is 5 of them (derived, not fitted).  The seed is fixed here and the restatement is
    checked against the bound on the CPU, so the GPU tests may rely on the same seed."""
    E, K, seed = 20000, CI.NUM_CLASSES, 20261020
    d = cdn_draws(seed, E, CI.W, K, 0.5, key_noise=True)
    flips = int(d.flip.sum())
    bound = 5.0 * math.sqrt(E * 0.25 * 0.75)
    print("flips %d of %d, expected %.0f +- %.1f" % (flips, E, E * 0.25, bound))
    assert abs(flips - E * 0.25) <= bound
    assert int(d.new_label.min()) >= 0 and int(d.new_label.max()) < K
    assert sorted(set(d.new_label[d.flip].tolist())) == list(range(K))       # every class occurs among the replaced labels
    assert set(d.sign.unique().tolist()) == {-1.0, 1.0}
    assert float(d.magnitude.min()) >= 0.0 and float(d.magnitude.max()) < 1.0
    assert abs(float(d.magnitude.mean()) - 0.5) < 5.0 / math.sqrt(12.0 * E * CI.W)      # uniform: sd of the mean
    assert abs(float(d.sign.mean())) < 5.0 / math.sqrt(E * CI.W)


# ---- the group arithmetic -------------------------------------------------------------------------------------------------
def test_group_arithmetic_branches():
    assert cdn_group_arithmetic((1,), 2) == (1, 4)                # doubled
    assert cdn_group_arithmetic((3, 1), 100) == (3, 33)           # 200 // 6
    assert cdn_group_arithmetic((3, 1), 50) == (3, 16)            # 100 >= 100: 100 // 6
    assert cdn_group_arithmetic((3, 1), 49) == (3, 98)            # 98 < 100: no division
    assert cdn_group_arithmetic((60, 2), 50) == (60, 1)           # 100 // 120 = 0, floored
    assert cdn_group_arithmetic((2, 0, 3), 0) == (3, 1)           # below 1
    assert cdn_group_arithmetic((0, 0), 7) == (0, 1)              # no target at all
    for case, c in CI.CASES.items():
        assert cdn_group_arithmetic(c["sizes"], c["dn"])[1] == CI.EXPECTED_GROUPS[case]


def test_all_empty_step_shapes():
    case = "empty_h8"
    label, key, mask, meta = prepare_for_cdn(CI.dn_args(case, CI.targets(case)), True, CI.QUERIES, CI.NUM_CLASSES, 8,
                                             CI.label_enc(case))
    assert tuple(label.shape) == (2, 0, 8) and tuple(key.shape) == (2, 0, CI.W)
    assert meta == {"pad_size": 0, "num_dn_group": 1}
    assert tuple(mask.shape) == (CI.QUERIES, CI.QUERIES) and not bool(mask.any())
    assert torch.equal(mask, cdn_attention_mask(0, 1, CI.QUERIES))


# ---- dn_post_process -------------------------------------------------------------------------------------------------------
def test_dn_post_process_slices_are_views():
    g = torch.Generator().manual_seed(5)
    layers, B, pad, Q = 3, 2, 8, 5
    mk = lambda d: torch.randn(layers, B, pad + Q, d, generator=g)
    cls, hand, obj = mk(14), mk(42), mk(42)
    mano, cam, objp = [mk(48), mk(10)], [mk(3), mk(3)], [mk(3), mk(1)]
    meta = {"pad_size": pad, "num_dn_group": 2}
    seen = []

    def set_aux(*a):
        seen.append(a)
        return "aux"
    out = dn_post_process(cls, hand, obj, mano, cam, objp, meta, True, set_aux)
    for got, src in zip(out[:3], (cls, hand, obj)):
        assert torch.equal(got, src[:, :, pad:]) and got.data_ptr() == src[:, :, pad:].data_ptr()       # a view, no copy
    for got, src in zip(out[3:], (mano, cam, objp)):
        assert isinstance(got, list) and len(got) == 2
        for gk, sk in zip(got, src):
            assert torch.equal(gk, sk[:, :, pad:]) and gk.data_ptr() == sk[:, :, pad:].data_ptr()
    known = meta["output_known_lbs_bboxes"]
    assert sorted(known) == ["aux_outputs", "pred_cams", "pred_hand_key", "pred_logits", "pred_mano_params", "pred_obj_key",
                             "pred_obj_params"]
    assert torch.equal(known["pred_logits"], cls[-1, :, :pad]) and known["pred_logits"].data_ptr() == cls[-1].data_ptr()
    assert torch.equal(known["pred_hand_key"], hand[-1, :, :pad]) and torch.equal(known["pred_obj_key"], obj[-1, :, :pad])
    for key, src in (("pred_mano_params", mano), ("pred_cams", cam), ("pred_obj_params", objp)):
        assert [torch.equal(a, s[-1, :, :pad]) for a, s in zip(known[key], src)] == [True, True]
    assert known["aux_outputs"] == "aux" and len(seen) == 1 and len(seen[0]) == 6
    assert torch.equal(seen[0][0], cls[:, :, :pad]) and torch.equal(seen[0][3][1], mano[1][:, :, :pad])
    # without denoising rows (evaluation, or an empty step) everything passes through untouched
    for m in (None, {"pad_size": 0, "num_dn_group": 1}):
        out = dn_post_process(cls, hand, obj, mano, cam, objp, m, True, set_aux)
        assert out[0] is cls and out[3] is mano and (m is None or "output_known_lbs_bboxes" not in m)
    meta2 = {"pad_size": pad, "num_dn_group": 2}
    dn_post_process(cls, hand, obj, mano, cam, objp, meta2, False, set_aux)
    assert "aux_outputs" not in meta2["output_known_lbs_bboxes"] and len(seen) == 1


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_entries_exported_and_in_table(lib):
    from uvhand_amd import _native
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    assert _native.SIGNATURES["msda_cdn_supported"] == "i ii ll"
    assert _native.SIGNATURES["msda_cdn_prepare_forward_f32"] == "i ppppp i l ii l iii u f pppp p"
    assert _native.SIGNATURES["msda_cdn_prepare_backward_f32"] == "i pp l i l p p"
    assert lib.msda_version() == 116


def test_supported_envelope(lib):
    ok = lib.msda_cdn_supported
    assert ok(256, 42, 92, 2 * 33 * 96) == 1
    assert ok(4, 1, 1, 0) == 1 and ok(1024, 64, 15, 100) == 1
    assert ok(6, 42, 15, 100) == 0 and ok(0, 42, 15, 100) == 0 and ok(1028, 42, 15, 100) == 0          # hidden
    assert ok(256, 0, 15, 100) == 0 and ok(256, 65, 15, 100) == 0                                         # width
    assert ok(256, 42, 0, 100) == 0 and ok(256, 42, 15, -1) == 0
    assert ok(256, 42, 1 << 23, 100) == 0                                                                 # rows_book * hidden = 2^31
    assert ok(256, 42, (1 << 23) - 1, 100) == 1
    last = (1 << 32) // (2 * 43)                                   # 2 E (1 + W) < 2^32
    assert ok(256, 42, 15, last) == 1 and ok(256, 42, 15, last + 1) == 0


def _fwd(lib, **kw):
    a = dict(labels=P, offsets=P, keys=P, weight=P, seed=P, B=2, T=5, W=42, H=256, rows=15, single_pad=3, groups=4, K=14, thr=0,
             scale=0.0, out_l=P, out_k=P, noised=P, dbg=None)
    a.update(kw)
    return lib.msda_cdn_prepare_forward_f32(a["labels"], a["offsets"], a["keys"], a["weight"], a["seed"], a["B"], a["T"], a["W"],
                                            a["H"], a["rows"], a["single_pad"], a["groups"], a["K"], a["thr"], a["scale"],
                                            a["out_l"], a["out_k"], a["noised"], a["dbg"], None)


def test_forward_argument_errors(lib):
    err = lambda: lib.msda_last_error().decode()
    assert _fwd(lib, B=-1) == ERR_ARGUMENT and _fwd(lib, T=-1) == ERR_ARGUMENT and _fwd(lib, single_pad=-1) == ERR_ARGUMENT
    assert _fwd(lib, groups=0) == ERR_ARGUMENT and _fwd(lib, K=0) == ERR_ARGUMENT
    assert _fwd(lib, scale=-0.5) == ERR_ARGUMENT and _fwd(lib, scale=float("nan")) == ERR_ARGUMENT
    assert "key_noise_scale" in err()
    assert _fwd(lib, H=6) == ERR_ARGUMENT and "msda_cdn_supported" in err()
    assert _fwd(lib, H=2048) == ERR_ARGUMENT and _fwd(lib, W=65) == ERR_ARGUMENT and _fwd(lib, W=0) == ERR_ARGUMENT
    assert _fwd(lib, T=1 << 24, groups=64) == ERR_ARGUMENT                      # counters beyond 2^32
    assert _fwd(lib, K=16) == ERR_ARGUMENT and "num_classes" in err()
    assert _fwd(lib, B=1 << 20, single_pad=1 << 10) == ERR_ARGUMENT and "2^31" in err()
    assert _fwd(lib, weight=None) == ERR_ARGUMENT and "null" in err()
    assert _fwd(lib, labels=None) == ERR_ARGUMENT and _fwd(lib, noised=None) == ERR_ARGUMENT and _fwd(lib, out_k=None) == ERR_ARGUMENT
    assert _fwd(lib, thr=1 << 30, seed=None) == ERR_ARGUMENT and "seed" in err()
    assert _fwd(lib, scale=0.4, seed=None) == ERR_ARGUMENT
    assert _fwd(lib, weight=P + 4) == ERR_ARGUMENT and "aligned" in err()
    assert _fwd(lib, out_l=P + 8) == ERR_ARGUMENT
    # nothing to do (no frame, or no target in any frame): no pointer is read, nothing is launched
    before = lib.msda_launch_count()
    assert _fwd(lib, B=0, labels=None, offsets=None, keys=None, weight=None, seed=None, out_l=None, out_k=None, noised=None) == 0
    assert _fwd(lib, single_pad=0, T=0, labels=None, keys=None, out_l=None, out_k=None, noised=None, seed=None) == 0
    assert lib.msda_launch_count() == before


def test_backward_argument_errors(lib):
    fn = lib.msda_cdn_prepare_backward_f32
    err = lambda: lib.msda_last_error().decode()
    assert fn(P, P, -1, 256, 15, P, None) == ERR_ARGUMENT
    assert fn(P, P, 48, 6, 15, P, None) == ERR_ARGUMENT and "multiple of 4" in err()
    assert fn(P, P, 48, 256, 0, P, None) == ERR_ARGUMENT
    assert fn(P, P, 1 << 23, 256, 15, P, None) == ERR_ARGUMENT                  # rows * hidden = 2^31
    assert fn(P, P, 48, 256, 15, None, None) == ERR_ARGUMENT and "null" in err()
    assert fn(None, P, 48, 256, 15, P, None) == ERR_ARGUMENT and fn(P, None, 48, 256, 15, P, None) == ERR_ARGUMENT
    assert fn(P + 4, P, 48, 256, 15, P, None) == ERR_ARGUMENT and "aligned" in err()
    assert fn(P, P, 48, 256, 15, P + 8, None) == ERR_ARGUMENT


def test_wrappers_and_drop_in_refuse_on_the_host():
    from uvhand_amd import _native
    with pytest.raises(RuntimeError):
        _native.cdn_prepare_forward(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 42),
                                    torch.zeros(15, 8), None, 1, 1, 14)
    with pytest.raises(RuntimeError):
        _native.cdn_prepare_backward(torch.zeros(1, 2, 8), torch.zeros(1, 2, dtype=torch.int32), 15)
    assert _native.cdn_flip_threshold(0.0) == 0 and _native.cdn_flip_threshold(0.5) == 1 << 30
    assert _native.cdn_flip_threshold(4.0) == 2 ** 32 - 1 and _native.cdn_flip_threshold(-1.0) == 0
