"""The attention cores' dropout stream (at_hash / at_mix, uvhand_amd/csrc/msda_attn_tile.h) tested like a random-number
generator, on the CPU: everything here works on tests/test_attention_gpu.py:_keep_mask, the numpy restatement of the hash.  The
kernels' own bits are tied to _keep_mask position by position in tests/test_attention_edges_gpu.py and
tests/test_attention_bf16_edges_gpu.py (the mask read back out of the forward, the backward through the p > 0 parity cases).

Every statistic is a standard score z = (observed - expected) / sigma under the hypothesis "independent keeps of probability
r = 1 - thresh / 2^32", and the bound is |z| <= 6 for each: a Bonferroni bound — 4 seeds x 2 rates x about 2 * 10^4 statistics
(9600 row counts, 9600 column counts, 32 pair counts, 496 pair-against-pair agreements, 6 shifts, 6 related seeds, the total) are
about 1.6 * 10^5 scores, which at a family-wise level of 10^-3 gives 5.8.  A hash with a 1 % dependence between two masks of
2.9 * 10^6 elements scores about 17.

Sigma.  A count of n keeps: n r (1 - r).  The agreement of two masks at n positions (rate A = r^2 + (1 - r)^2): n A (1 - A) when
no element takes part in two comparisons (two pairs, two seeds).  The agreement of a mask with itself shifted by d along an
axis of length L compares every element with both of its neighbours at distance d, and for r != 1/2 two comparisons that share an
element are correlated, cov = r^3 + (1 - r)^3 - A^2; a line of L elements has L - d comparisons and max(L - 2d, 0) such
neighbours, so sigma^2 = lines * ((L - d) A (1 - A) + 2 max(L - 2d, 0) cov)."""
import numpy as np
import pytest

from test_attention_gpu import _keep_mask

SEEDS = (0x1234567890ABCDEF, 77, 0, 0xFFFFFFFFFFFFFFFF)
RATES = (0.1, 0.5)
PAIRS, LQ, LK = 32, 300, 300
BOUND = 6.0
M64 = (1 << 64) - 1
WORST = {}


def _keep_rate(p):
    thresh = int(np.uint32(min(4294967295.0, float(np.float32(p)) * 4294967296.0)))
    return 1.0 - thresh / 4294967296.0


def _unrelated(seed):
    return (seed * 6364136223846793005 + 1442695040888963407) & M64


_MASKS = {}


def _mask(seed, p):
    key = (seed & M64, p)
    if key not in _MASKS:
        m = _keep_mask(seed & M64, PAIRS, LQ, LK, p)
        m.setflags(write=False)                          # (computed once per seed and rate, shared by the tests, left unchanged)
        _MASKS[key] = m
    return _MASKS[key]


def _score(name, observed, expected, sigma):
    z = np.abs((np.asarray(observed, np.float64) - expected) / sigma)
    worst = float(z.max())
    WORST[name] = max(WORST.get(name, 0.0), worst)
    return worst


def _check(what, name, observed, expected, sigma):
    worst = _score(name, observed, expected, sigma)
    print("%s %-28s worst |z| %.2f" % (what, name, worst))
    assert worst <= BOUND, (what, name, worst)


def _agree_sigma(r, n):
    a = r * r + (1 - r) * (1 - r)
    return a, np.sqrt(n * a * (1 - a))


def _shift_sigma(r, lines, length, d):
    a = r * r + (1 - r) * (1 - r)
    cov = r ** 3 + (1 - r) ** 3 - a * a
    return a, np.sqrt(lines * ((length - d) * a * (1 - a) + 2 * max(length - 2 * d, 0) * cov))


CASES = [(s, p) for s in SEEDS for p in RATES]


@pytest.mark.parametrize("seed,p", CASES)
def test_keep_counts(seed, p):
    what = "seed %#x p=%g" % (seed, p)
    m, r = _mask(seed, p), _keep_rate(p)
    var1 = r * (1 - r)
    _check(what, "row count", m.sum(2), LK * r, np.sqrt(LK * var1))
    _check(what, "column count", m.sum(1), LQ * r, np.sqrt(LQ * var1))
    _check(what, "pair count", m.sum((1, 2)), LQ * LK * r, np.sqrt(LQ * LK * var1))
    _check(what, "total count", m.sum(), m.size * r, np.sqrt(m.size * var1))


@pytest.mark.parametrize("seed,p", CASES)
def test_a_mask_does_not_follow_its_own_neighbours(seed, p):
    what = "seed %#x p=%g" % (seed, p)
    m, r = _mask(seed, p), _keep_rate(p)
    for axis, label, length, shifts in ((2, "keys", LK, (1, 16)), (1, "queries", LQ, (1, 16)), (0, "pairs", PAIRS, (1, 8))):
        for d in shifts:
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, length - d), slice(d, length)
            a, sigma = _shift_sigma(r, m.size // length, length, d)
            agree = int((m[tuple(lo)] == m[tuple(hi)]).sum())
            _check(what, "shift %d along %s" % (d, label), agree, (m.size // length) * (length - d) * a, sigma)


@pytest.mark.parametrize("seed,p", CASES)
def test_pairs_are_independent_of_each_other(seed, p):
    what = "seed %#x p=%g" % (seed, p)
    m, r = _mask(seed, p), _keep_rate(p)
    n = LQ * LK
    a, sigma = _agree_sigma(r, n)
    flat = m.reshape(PAIRS, n)
    agree = [int((flat[i] == flat[j]).sum()) for i in range(PAIRS) for j in range(i + 1, PAIRS)]
    assert len(agree) == PAIRS * (PAIRS - 1) // 2
    _check(what, "pair against pair", agree, n * a, sigma)


@pytest.mark.parametrize("seed,p", CASES)
def test_related_seeds_give_unrelated_masks(seed, p):
    what = "seed %#x p=%g" % (seed, p)
    m, r = _mask(seed, p), _keep_rate(p)
    a, sigma = _agree_sigma(r, m.size)
    others = (("s ^ 1", seed ^ 1), ("s ^ (1 << 16)", seed ^ (1 << 16)), ("s ^ (1 << 32)", seed ^ (1 << 32)),
              ("s ^ (1 << 63)", seed ^ (1 << 63)), ("s + 1", (seed + 1) & M64), ("unrelated seed", _unrelated(seed)))
    for label, other in others:
        assert other != seed
        agree = int((m == _keep_mask(other, PAIRS, LQ, LK, p)).sum())
        _check(what, "against " + label, agree, m.size * a, sigma)


def test_the_restated_rate_and_the_no_dropout_mask():
    """What the scores above take for granted: p = 0 keeps everything, the rate is the threshold's."""
    assert _keep_mask(5, 2, 3, 4, 0.0).all()
    assert _keep_rate(0.5) == 0.5 and abs(_keep_rate(0.1) - 0.9) < 2.0 ** -26
    assert not _keep_mask(0x1234567890ABCDEF, 4, 320, 320, 1.0 - 2.0 ** -24).any()      # thresh 2^32 - 256


def test_zz_print_worst_scores():
    for k in sorted(WORST):
        print("worst |z| %-28s %.2f" % (k, WORST[k]))
