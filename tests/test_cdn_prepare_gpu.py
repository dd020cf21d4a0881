"""prepare_for_cdn on the GPU (uvhand_amd/utils/denoising.py, functions/cdn_func.py, csrc/msda_cdn.hip): the one-launch forward
against the reference's fixture (no tolerance: layout, labels, embedding rows, padding) and against the composition fed with the
restated draws (no tolerance: labels and the noised keys before inverse_sigmoid), the keys after inverse_sigmoid and the weight
gradient under the project's fp64 rule, reproducibility, launch counts, torch.cuda.set_sync_debug_mode("error"), graph replay on
fresh targets, and the outputs driven through DinoTransformerDecoder."""
import gc
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cdn_prepare_inputs as CI  # noqa: E402
import dino_inputs as DI  # noqa: E402

pytestmark = pytest.mark.gpu

RATIOS = {}
F32, F64 = torch.float32, torch.float64
BIG = dict(sizes=(16, 5), dn=100, hidden=256, seed=5201)             # B = 2, 200 // 32 = 6 groups, pad 192
# (sizes, dn, hidden, W): 1188 rows = two chunks of the backward's compaction; hidden 8 / 12 / 256 / 1024 = 128 / 85 (idle
# threads) / 4 / 1 summing groups and 1 .. 4 float4 per lane of the forward; W = 1, 42, 64 (the widest)
KERNEL_SHAPES = [((3, 1, 2, 0, 3, 1), 100, 8, 42), ((3, 1, 2, 0, 3, 1), 100, 12, 1), ((3, 1, 2, 0, 3, 1), 100, 256, 64),
                 ((3, 1, 2, 0, 3, 1), 100, 1024, 42), ((16, 5), 100, 256, 42)]


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return load_golden("cdn_prepare")


def _targets(sizes, seed, W=CI.W, dtype=F32):
    tg = CI.make_targets(sizes, seed, _dev(), dtype)
    if W != CI.W:
        tg["keypoints"] = [torch.cat([k, k], 1)[:, :W].contiguous() for k in tg["keypoints"]]
    return tg


def _index_enc():
    """An embedding whose row i is [i + 1]: the composition's input_query_label then spells the noised labels (0 = padding)."""
    enc = nn.Embedding(CI.NUM_CLASSES + 1, 1)
    with torch.no_grad():
        enc.weight.copy_(torch.arange(1, CI.NUM_CLASSES + 2, dtype=F32)[:, None])
    return enc.to(_dev())


def _oracle(tg, dn, ratio, box, enc, hidden, seed, key_noise, raw_keys=False):
    """The composition fed with the kernel's draws for ``seed``; raw_keys: inverse_sigmoid replaced by the identity, which leaves
    the noised, clamped keys in the second output."""
    from uvhand_amd.functions import dino_func
    from uvhand_amd.utils import cdn_draws, cdn_group_arithmetic, prepare_for_cdn_composition
    sizes = tuple(len(l) for l in tg["labels"])
    _, groups = cdn_group_arithmetic(sizes, dn)
    W = tg["keypoints"][0].shape[1]
    draws = cdn_draws(seed, 2 * groups * sum(sizes), W, CI.NUM_CLASSES, ratio, key_noise=key_noise and box > 0)
    real = dino_func.inverse_sigmoid
    if raw_keys:
        dino_func.inverse_sigmoid = lambda x: x
    try:
        return prepare_for_cdn_composition((tg, dn, ratio, box), True, CI.QUERIES, CI.NUM_CLASSES, hidden, enc, key_noise=key_noise,
                                           draws=draws)
    finally:
        dino_func.inverse_sigmoid = real


def _node(tg, dn, ratio, box, enc, seed, key_noise):
    from uvhand_amd.functions.cdn_func import cdn_prepare
    from uvhand_amd.utils import cdn_group_arithmetic
    from uvhand_amd.utils.denoising import _pack
    packed = _pack(tg, _dev())
    single_pad, groups = cdn_group_arithmetic(packed.sizes, dn)
    return cdn_prepare(enc.weight, packed.labels, packed.offsets, packed.keypoints, single_pad, groups, CI.NUM_CLASSES, ratio,
                       box if key_noise else 0.0, seed=seed, key_debug=True)


# ---- ratio 0: the reference's fixture, no tolerance -------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CI.SMALL if CI.CASES[c]["ratio"] == 0.0])
def test_ratio_zero_equals_the_fixture(case, golden):
    from uvhand_amd import _native as MSDA
    from uvhand_amd.utils import prepare_for_cdn
    c = CI.CASES[case]
    enc, tg = CI.label_enc(case, _dev()), CI.targets(case, _dev())
    n0 = MSDA.launch_count()
    label, key, mask, meta = prepare_for_cdn(CI.dn_args(case, tg), True, CI.QUERIES, CI.NUM_CLASSES, c["hidden"], enc)
    launches = MSDA.launch_count() - n0
    assert meta == {"pad_size": int(golden[case + "/meta"][0]), "num_dn_group": int(golden[case + "/meta"][1])}
    assert np.array_equal(mask.cpu().numpy(), golden[case + "/mask"])
    assert np.array_equal(label.detach().cpu().numpy(), golden[case + "/label"])         # weight[labels] bit for bit, zero padding
    assert tuple(key.shape) == golden[case + "/key"].shape
    if sum(c["sizes"]) == 0:
        assert launches == 0 and label.shape[1] == 0                                      # the all-empty step launches nothing
        return
    assert launches == 1
    # the labels and the layout, spelled out: row r * single_pad + j of frame b is target j of that frame, the rest padding
    noised = _node(tg, c["dn"], 0.0, 0.0, enc, None, False)[2].cpu()
    single_pad, reps = max(c["sizes"]), 2 * meta["num_dn_group"]
    want = torch.full((len(c["sizes"]), meta["pad_size"]), -1, dtype=torch.int32)
    for b, frame in enumerate(tg["labels"]):
        for r in range(reps):
            for j, lab in enumerate(frame):
                want[b, r * single_pad + j] = lab
    assert torch.equal(noised, want)
    pad_rows = want < 0
    assert not bool(label.detach().cpu()[pad_rows].any()) and not bool(key.cpu()[pad_rows].any())     # exactly zero
    assert torch.equal(label.detach().cpu()[~pad_rows], enc.weight.detach().cpu()[want[~pad_rows].long()])
    # the keys after inverse_sigmoid: the fp64 rule, the fixture being the fp32 torch composition
    tg64, enc64 = CI.targets(case, _dev(), F64), CI.label_enc(case, _dev(), F64)
    from uvhand_amd.utils import prepare_for_cdn_composition
    l64, k64, _, _ = prepare_for_cdn_composition(CI.dn_args(case, tg64), True, CI.QUERIES, CI.NUM_CLASSES, c["hidden"], enc64)
    k32 = prepare_for_cdn_composition(CI.dn_args(case, tg), True, CI.QUERIES, CI.NUM_CLASSES, c["hidden"], enc)[1]
    CI.hold(case + " input_query_key", key, k32, k64, RATIOS)
    # the weight gradient of the fixture's weighted sum
    CI.loss_of(label, key, c["seed"] + 2).backward()
    g32 = torch.from_numpy(golden[case + "/grad_weight"]).to(_dev())
    CI.loss_of(l64, k64, c["seed"] + 2).backward()
    CI.hold(case + " grad_weight (fixture)", enc.weight.grad, g32, enc64.weight.grad, RATIOS)


# ---- draws: the composition with the restated hash, no tolerance ----------------------------------------------------------------
@pytest.mark.parametrize("key_noise", [False, True])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "B%d_H%d_W%d" % (len(s[0]), s[2], s[3]))
def test_draws_equal_the_composition_with_restated_draws(shape, key_noise):
    sizes, dn, hidden, W = shape
    ratio, box = 0.5, 0.4
    tg = _targets(sizes, 5300 + hidden + W, W)
    enc = CI.make_label_enc(hidden, 5400 + hidden, _dev())
    seed = torch.tensor([0x5DEECE66D1234567 + hidden], dtype=torch.int64, device=_dev())
    label, key, noised, raw = _node(tg, dn, ratio, box, enc, seed, key_noise)
    want_idx = _oracle(tg, dn, ratio, box, _index_enc(), 1, seed, key_noise)[0]
    want_noised = (want_idx[..., 0] - 1).to(torch.int32)
    assert torch.equal(noised, want_noised)
    plain = _oracle(tg, dn, 0.0, box, _index_enc(), 1, seed, False)[0]
    assert 0 < int((want_idx != plain).sum()) < int((plain > 0).sum())                  # some labels flipped, not all
    want_label, want_key, _, _ = _oracle(tg, dn, ratio, box, enc, hidden, seed, key_noise)
    assert torch.equal(label.detach(), want_label.detach())                               # embedding rows, zero padding
    want_raw = _oracle(tg, dn, ratio, box, enc, hidden, seed, key_noise, raw_keys=True)[1]
    assert torch.equal(raw, want_raw)                                                     # before inverse_sigmoid: bit for bit
    assert float(raw.min()) >= 0.0 and float(raw.max()) <= 1.0
    src = _oracle(tg, dn, 0.0, 0.0, enc, hidden, seed, False, raw_keys=True)[1]
    assert torch.equal(raw, src) != key_noise                                             # the noise is there iff asked for
    # after inverse_sigmoid, and the weight gradient against torch's own embedding backward: the fp64 rule
    tg64 = dict(tg, keypoints=[k.double() for k in tg["keypoints"]])
    enc64 = CI.make_label_enc(hidden, 5400 + hidden, _dev(), F64)
    l64, k64, _, _ = _oracle(tg64, dn, ratio, box, enc64, hidden, seed, key_noise)
    what = "B%d H%d W%d%s" % (len(sizes), hidden, W, " key_noise" if key_noise else "")
    CI.hold(what + " input_query_key", key, want_key, k64, RATIOS)
    for out, k_, e_ in ((label, key, enc), (want_label, want_key, enc), (l64, k64, enc64)):
        e_.weight.grad = None
        CI.loss_of(out, k_, 77).backward()
        if out is label:
            ours = e_.weight.grad.clone()
    CI.hold(what + " grad_weight", ours, enc.weight.grad, enc64.weight.grad, RATIOS)
    assert float(ours[CI.NUM_CLASSES].abs().max()) == 0.0                                 # a row no label selects: written as zero


def test_prepare_for_cdn_draws_from_one_device_seed():
    """The drop-in's seed is one random_() on a device scalar under torch's seed: redrawing it gives the oracle's input."""
    from uvhand_amd.utils import prepare_for_cdn
    sizes, dn, hidden = BIG["sizes"], BIG["dn"], BIG["hidden"]
    tg, enc = _targets(sizes, BIG["seed"]), CI.make_label_enc(hidden, BIG["seed"] + 1, _dev())
    for key_noise in (False, True):
        torch.manual_seed(99)
        label, key, mask, meta = prepare_for_cdn((tg, dn, 0.5, 0.4), True, CI.QUERIES, CI.NUM_CLASSES, hidden, enc, key_noise=key_noise)
        torch.manual_seed(99)
        seed = torch.empty(1, dtype=torch.int64, device=_dev()).random_()
        want_label, want_key, want_mask, want_meta = _oracle(tg, dn, 0.5, 0.4, enc, hidden, seed, key_noise)
        assert meta == want_meta == {"pad_size": 192, "num_dn_group": 6} and torch.equal(mask, want_mask)
        assert torch.equal(label.detach(), want_label.detach())
        tg64 = dict(tg, keypoints=[k.double() for k in tg["keypoints"]])
        k64 = _oracle(tg64, dn, 0.5, 0.4, CI.make_label_enc(hidden, BIG["seed"] + 1, _dev(), F64), hidden, seed, key_noise)[1]
        CI.hold("drop-in key_noise=%s input_query_key" % key_noise, key, want_key, k64, RATIOS)
    torch.manual_seed(100)
    other = prepare_for_cdn((tg, dn, 0.5, 0.4), True, CI.QUERIES, CI.NUM_CLASSES, hidden, enc)[0]
    assert not torch.equal(other, label)


# ---- reproducibility, launches, syncs -------------------------------------------------------------------------------------------
def _big_weights():
    """The loss weights of BIG's outputs, made before a region that must not touch the host (a blocking copy synchronises)."""
    return CI.output_weights(78, [(2, 192, BIG["hidden"]), (2, 192, CI.W)], _dev())


def _step(tg, enc, weights, packed=None, ratio=0.5, key_noise=True):
    from uvhand_amd.utils import prepare_for_cdn
    label, key, _, _ = prepare_for_cdn((tg, BIG["dn"], ratio, 0.4), True, CI.QUERIES, CI.NUM_CLASSES, BIG["hidden"], enc,
                                       packed=packed, key_noise=key_noise)
    ((label * weights[0]).sum() + (key * weights[1]).sum()).backward()
    return label, key


def test_grad_weight_is_bitwise_reproducible():
    tg, enc = _targets(BIG["sizes"], BIG["seed"]), CI.make_label_enc(BIG["hidden"], BIG["seed"] + 1, _dev())
    grads, weights = [], _big_weights()
    for det in (False, False, True):
        torch.use_deterministic_algorithms(det)
        try:
            enc.weight.grad = None
            torch.manual_seed(5)
            _step(tg, enc, weights)
            grads.append(enc.weight.grad.clone())
        finally:
            torch.use_deterministic_algorithms(False)
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


def test_one_launch_each_way_and_no_host_sync(monkeypatch):
    from uvhand_amd import _native as MSDA
    from uvhand_amd.functions import cdn_func
    tg, enc = _targets(BIG["sizes"], BIG["seed"]), CI.make_label_enc(BIG["hidden"], BIG["seed"] + 1, _dev())
    weights = _big_weights()
    _step(tg, enc, weights)                                  # first call: module load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n0 = MSDA.launch_count()
        from uvhand_amd.utils import prepare_for_cdn
        label, key, _, _ = prepare_for_cdn((tg, BIG["dn"], 0.5, 0.4), True, CI.QUERIES, CI.NUM_CLASSES, BIG["hidden"], enc, key_noise=True)
        n1 = MSDA.launch_count()
        ((label * weights[0]).sum() + (key * weights[1]).sum()).backward()
        n2 = MSDA.launch_count()
        monkeypatch.setattr(cdn_func, "FUSED", False)
        with pytest.raises(RuntimeError):
            _step(tg, enc, weights)                                   # the reference's nonzero over the drawn selection
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert (n1 - n0, n2 - n1) == (1, 1)
    assert bool(torch.isfinite(enc.weight.grad).all())


def test_other_inputs_take_the_composition():
    """What the kernels do not take runs the composition: no library launch, same values."""
    from uvhand_amd import _native as MSDA
    from uvhand_amd.utils import prepare_for_cdn
    tg = _targets((2, 3), 5501)
    plain = CI.make_label_enc(8, 5502, _dev())
    want = prepare_for_cdn((tg, 2, 0.0, 0.0), True, CI.QUERIES, CI.NUM_CLASSES, 8, plain)[0]
    padded = nn.Embedding(CI.NUM_CLASSES + 1, 8, padding_idx=0).to(_dev())
    hooked = CI.make_label_enc(8, 5502, _dev())
    hooked.register_forward_hook(lambda m, i, o: None)
    with torch.no_grad():
        padded.weight.copy_(plain.weight)
    n0 = MSDA.launch_count()
    for enc, targets in ((padded, tg), (hooked, tg), (CI.make_label_enc(8, 5502, _dev(), F64), tg)):
        got = prepare_for_cdn((targets, 2, 0.0, 0.0), True, CI.QUERIES, CI.NUM_CLASSES, 8, enc)[0]
        assert torch.equal(got.float(), want)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = prepare_for_cdn((tg, 2, 0.0, 0.0), True, CI.QUERIES, CI.NUM_CLASSES, 8, plain)[0]
    assert torch.equal(got.float(), want)
    assert MSDA.launch_count() == n0
    with pytest.raises(IndexError):
        prepare_for_cdn((dict(tg, labels=[[1, 99], [0, 1, 2]]), 2, 0.0, 0.0), True, CI.QUERIES, CI.NUM_CLASSES, 8, plain)
    assert MSDA.launch_count() == n0


# ---- graph ------------------------------------------------------------------------------------------------------------------
def test_step_replays_from_one_graph_on_fresh_targets():
    """Forward + backward captured once over the packed buffers; new labels and keypoints of the same frame sizes are copied into
    them and the replay equals the eager step on those targets bit for bit.  Twice: the drop-in at ratio 0, and the node with a
    seed buffer at ratio 0.5 with key noise (the drop-in's own seed is a random_() of torch's generator, whose captured offset an
    eager call does not share)."""
    from uvhand_amd.functions.cdn_func import cdn_prepare
    from uvhand_amd.utils import cdn_group_arithmetic, prepare_for_cdn
    from uvhand_amd.utils.denoising import _pack
    sizes, dn, hidden = BIG["sizes"], BIG["dn"], BIG["hidden"]
    enc = CI.make_label_enc(hidden, BIG["seed"] + 1, _dev())
    tg_a, tg_b = _targets(sizes, 5601), _targets(sizes, 5602)
    packed = _pack(tg_a, _dev())
    single_pad, groups = cdn_group_arithmetic(sizes, dn)
    seed = torch.tensor([123456789], dtype=torch.int64, device=_dev())
    weights = _big_weights()

    def drop_in(tg, pk):
        label, key, _, _ = prepare_for_cdn((tg, dn, 0.0, 0.4), True, CI.QUERIES, CI.NUM_CLASSES, hidden, enc, packed=pk)
        ((label * weights[0]).sum() + (key * weights[1]).sum()).backward()
        return label, key

    def node(tg, pk):
        label, key = cdn_prepare(enc.weight, pk.labels, pk.offsets, pk.keypoints, single_pad, groups, CI.NUM_CLASSES, 0.5, 0.4,
                                 seed=seed)[:2]
        ((label * weights[0]).sum() + (key * weights[1]).sum()).backward()
        return label, key

    for step in (drop_in, node):
        packed.labels.copy_(_pack(tg_a, _dev()).labels)
        packed.keypoints.copy_(torch.cat(tg_a["keypoints"]))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step(tg_a, packed)
        torch.cuda.current_stream().wait_stream(side)
        enc.weight.grad = None
        gc.collect()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step(tg_a, packed)
        fresh = _pack(tg_b, _dev())
        packed.labels.copy_(fresh.labels)
        packed.keypoints.copy_(fresh.keypoints)
        seed.add_(1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.detach().clone() for o in outs] + [enc.weight.grad.clone()]
        enc.weight.grad = None
        eager = step(tg_b, fresh)
        eager = [o.detach() for o in eager] + [enc.weight.grad]
        assert [tuple(a.shape) for a in replayed] == [tuple(b.shape) for b in eager]
        for i, (a, b) in enumerate(zip(replayed, eager)):
            assert torch.equal(a, b), (step.__name__, i)
        assert not torch.equal(replayed[0], step(tg_a, _pack(tg_a, _dev()))[0].detach())            # the targets did change
        enc.weight.grad = None
        del graph


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_outputs_drive_the_dino_decoder_sync_free():
    """The denoising rows in front of seeded matching queries through DinoTransformerDecoder at its fixture shape under the
    returned mask: forward + backward without a host sync, and label_enc is trained through the decoder."""
    from uvhand_amd.modules import DinoDeformableTransformerDecoderLayer, DinoTransformerDecoder
    from uvhand_amd.utils import prepare_for_cdn
    c = DI.CFG
    dec = DI.build(DinoDeformableTransformerDecoderLayer, DinoTransformerDecoder, "w42").to(_dev())
    prep = DI.prepare("w42", _dev(), ref_grad=False)
    enc = CI.make_label_enc(c["d"], 5701, _dev())
    tg = _targets((c["single_pad"], 1), 5702)                   # N = 2 frames, single_pad 2; dn_number 1 is used as 2 groups
    g = torch.Generator().manual_seed(5703)
    q_tgt = torch.randn(c["N"], c["queries"], c["d"], generator=g).to(_dev())
    q_ref = torch.randn(c["N"], c["queries"], 42, generator=g).to(_dev())

    def step():
        label, key, mask, meta = prepare_for_cdn((tg, 1, 0.5, 0.4), True, c["queries"], CI.NUM_CLASSES, c["d"], enc, key_noise=True)
        assert meta == {"pad_size": 2 * c["single_pad"] * c["dn_number"], "num_dn_group": c["dn_number"]}
        prep["leaves"]["tgt"] = torch.cat([label, q_tgt], 1).transpose(0, 1)
        prep["leaves"]["refpoints"] = torch.cat([key, q_ref], 1).transpose(0, 1)
        prep["kwargs"]["tgt_mask"] = mask
        return DI.step(dec, prep)

    step()                                                       # warm-up: module loads, MSDeformAttn's one-time shape check
    torch.cuda.synchronize()
    enc.weight.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    grad = enc.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0


def test_zz_print_ratios():
    for k in sorted(RATIOS):
        print("worst ratio %-60s %.2f" % (k, RATIOS[k]))
