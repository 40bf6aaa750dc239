"""The int8 screen's key bound with the query credit, restated in numpy (no GPU).

The screen key of row x for query q is ``s t <c, b> + beta ||q||``: (s, c) the row's bf16 scale and
int8 codes, ``beta = ||x - s c|| + eps_d ||s c||`` rounded up to bf16 (k_quant_rows), (t, b) the
query's scale and codes (k_pack_qtile_i8).  The refine adds the per-query margin ``qeps``:

    true <x, q> <= s t <c, b> + beta ||q|| + qeps[q]

where ``qeps = X max(0, over) - Xmin max(0, -over) + slop``, ``over = ||q - t b|| - eps_d ||q||``,
X / Xmin the largest / smallest ``||s c||`` of the corpus.  A query whose own error is below the
share ``eps_d ||q||`` the rows carry has ``qeps < 0``: the credit.  This file restates the three
pieces with the kernels' rounding rules and checks the inequality in fp64 for every (row, query)
pair: random rows, rows of norms 1e-2 .. 1e2, a zero row, d in {64, 512, 1536}, and adversarial
rows whose true score sits on their bound (error parallel to a flat query).
"""
import math

import numpy as np
import pytest

F32, F64 = np.float32, np.float64


def eps_d(d):
    return 1.1 * math.sqrt(2.0 * math.log(2.0 * max(d, 1))) / (127.0 * 3.4641016151377544)


def f32_up(v):  # smallest fp32 >= v, either sign
    f = np.asarray(v, F64).astype(F32)
    return np.where(f.astype(F64) < v, np.nextafter(f, F32(np.inf)), f).astype(F32)


def f32_down(v):  # largest fp32 <= v
    f = np.asarray(v, F64).astype(F32)
    return np.where(f.astype(F64) > v, np.nextafter(f, F32(-np.inf)), f).astype(F32)


def bf16_rne_bits(f):
    u = np.asarray(f, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)


def bf16_up_bits(f):  # smallest bf16 >= f (f >= 0)
    u = np.asarray(f, F32).view(np.uint32)
    return (u >> 16) + ((u & 0xFFFF) != 0)


def bf16_bits_to_f32(b):
    return (np.asarray(b, np.uint32) << 16).view(F32)


def quant_rows(x):
    """k_quant_rows on stored fp32 values: scale, codes, beta per row; X, B, Xmin over the rows."""
    d = x.shape[1]
    x64 = x.astype(F64)
    mx = np.abs(x).max(axis=1).astype(F32)
    s = bf16_bits_to_f32(bf16_rne_bits(mx / F32(127.0)))
    s64 = s.astype(F64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(s64 > 0, np.clip(np.rint(x64 / s64), -127, 127), 0.0)
    e2 = ((x64 - s64 * c) ** 2).sum(axis=1)
    xh = np.sqrt((c * c).sum(axis=1)) * s.astype(F64)
    beta = bf16_bits_to_f32(bf16_up_bits(f32_up((np.sqrt(e2) + eps_d(d) * xh) * (1.0 + 1e-9))))
    X = f32_up(xh * (1.0 + 1e-9)).max()
    Xmin = f32_down(xh * (1.0 - 1e-9)).min()
    return s, c, beta, F64(X), F64(beta.max()), F64(Xmin)


def pack_query(q, X, B, Xmin, credit=True):
    """k_pack_qtile_i8 (inner product, no group means) for one fp32 query: t, codes, qeps, over."""
    d = q.shape[0]
    mx = F32(np.abs(q).max())
    t = F32(mx / F32(127.0))
    inv = F32(1.0) / t if t > 0 else F32(0.0)
    b = np.clip(np.rint((q * inv).astype(F32)), -127, 127).astype(F64)
    q64 = q.astype(F64)
    e2 = ((q64 - F64(t) * b) ** 2).sum()
    n2 = (q64 * q64).sum()
    c2 = (b * b).sum()
    qn = F64(f32_up(math.sqrt(n2) * (1.0 + 1e-9)))
    eq = math.sqrt(e2) * (1.0 + 1e-9)
    qh = math.sqrt(c2) * F64(t) * (1.0 + 1e-9)
    slop = 8.0 * 2.0 ** -24 * (X * qh + B * qn) + 1e-30
    over = eq - eps_d(d) * math.sqrt(n2) * (1.0 - 1e-9)
    e = X * max(0.0, over) + slop
    cr = Xmin * -over * (1.0 - 1e-9) if (credit and t > 0 and over < 0 and np.isfinite(Xmin)) else 0.0
    qeps = F64(f32_up(e * (1.0 + 1e-9) - cr))
    return F64(t), b, qeps, over


def flat_query(d, rng):
    sig = rng.choice([-1.0, 1.0], size=d)
    return (sig / math.sqrt(d)).astype(F32), sig


def adversarial_rows(sig, n, rng, log2s=-10):
    """x_i = s (c_i + sign(q_i) / 4), s a power of two, |c_i| <= 31, one coordinate at 127 s pinning the
    scale: bf16-exact values whose int8 error is s / 4 in the flat query's direction on every other
    coordinate, so <x - s c, q> = ||x - s c|| ||q|| up to that one coordinate."""
    d = sig.shape[0]
    s = 2.0 ** log2s
    m = rng.integers(0, 32, size=(n, d)).astype(F64)
    x = s * (sig[None, :] * m + 0.25 * sig[None, :])
    x[:, 0] = 127.0 * s * sig[0]
    return x.astype(F32)


def check_all_pairs(x, queries, credit=True):
    s, c, beta, X, B, Xmin = quant_rows(x)
    x64 = x.astype(F64)
    out = []
    for q in queries:
        t, b, qeps, over = pack_query(q, X, B, Xmin, credit)
        q64 = q.astype(F64)
        true = x64 @ q64
        bound = s.astype(F64) * t * (c @ b) + beta.astype(F64) * math.sqrt((q64 * q64).sum()) + qeps
        assert np.all(true <= bound), float((true - bound).max())
        out.append((qeps, over, float((bound - true).min())))
    return out, Xmin


def queries_for(d, rng):
    g = rng.standard_normal((6, d))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    flat, sig = flat_query(d, rng)
    spiky = np.full(d, 1.0)
    spiky[d // 3] = 50.0
    spiky /= np.linalg.norm(spiky)
    qs = [r.astype(F32) for r in g] + [np.zeros(d, F32), flat, spiky.astype(F32), (7.5 * g[0]).astype(F32)]
    return qs, sig


def test_rounding_helpers():
    for v in (1.0 + 1e-12, -1.0 - 1e-12, -1e-3 * (1 + 1e-10), 3e-39, -3e-39):
        assert float(f32_up(v)) >= v and float(np.nextafter(f32_up(v), F32(-np.inf))) < v
        assert float(f32_down(v)) <= v and float(np.nextafter(f32_down(v), F32(np.inf))) > v
    assert bf16_bits_to_f32(bf16_up_bits(F32(1.0))) == 1.0
    assert bf16_bits_to_f32(bf16_up_bits(np.nextafter(F32(1.0), F32(2.0)))) == F32(1.0078125)


@pytest.mark.parametrize("d", [64, 512, 1536])
def test_bound_holds_random_and_scaled_rows(d):
    rng = np.random.default_rng(100 + d)
    qs, _ = queries_for(d, rng)
    x = rng.standard_normal((300, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x *= 10.0 ** rng.uniform(-2.0, 2.0, size=(300, 1))  # norms 1e-2 .. 1e2
    x = np.concatenate([x, rng.standard_normal((40, d)) / math.sqrt(d)])
    res, Xmin = check_all_pairs(x.astype(F32), qs)
    off, _ = check_all_pairs(x.astype(F32), qs, credit=False)
    assert Xmin > 0
    # the credit is there: Gaussian queries (and the flat one) have less error than the rows' share,
    # and their margin drops by Xmin x the deficit (these rows' norms spread over 1e4, so the fp32
    # slop of the largest may still outweigh it: the margin's sign is not asserted here)
    for i in list(range(6)) + [7, 9]:
        assert res[i][1] < 0 and res[i][0] < off[i][0]
        assert res[i][0] <= off[i][0] - 0.99 * Xmin * -res[i][1]
    assert min(res[i][1] for i in range(9)) == res[7][1]  # flat: the largest deficit of the unit queries
    assert res[6][0] == off[6][0] > 0  # zero query: no credit
    assert res[8][1] > 0 and res[8][0] == off[8][0] > 0  # spiky: the excess branch


@pytest.mark.parametrize("d", [64, 512, 1536])
def test_unit_rows_margin_is_negative(d):
    """Unit-norm rows (the flagship's): the credit outweighs the slop and the margin is negative."""
    rng = np.random.default_rng(150 + d)
    qs, _ = queries_for(d, rng)
    x = rng.standard_normal((300, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    res, Xmin = check_all_pairs(x.astype(F32), qs)
    assert 0.98 < Xmin < 1.02
    assert all(res[i][0] < 0 for i in list(range(6)) + [7, 9])
    assert res[6][0] > 0 and res[8][0] > 0


@pytest.mark.parametrize("d", [64, 512, 1536])
def test_zero_row_gives_no_credit(d):
    rng = np.random.default_rng(200 + d)
    qs, _ = queries_for(d, rng)
    x = rng.standard_normal((50, d)).astype(F32)
    x[17] = 0.0
    res, Xmin = check_all_pairs(x, qs)
    assert Xmin == 0.0
    on = [r[0] for r in res]
    off = [r[0] for r in check_all_pairs(x, qs, credit=False)[0]]
    assert on == off and all(v > 0 for v in on)


@pytest.mark.parametrize("d", [64, 512, 1536])
def test_adversarial_rows_sit_on_their_bound(d):
    rng = np.random.default_rng(300 + d)
    qs, sig = queries_for(d, rng)
    adv = adversarial_rows(sig, 64, rng)
    # alone (Xmin is their own ||s c||, within their spread) and among unit Gaussian rows
    g = rng.standard_normal((200, d))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    for x in (adv, np.concatenate([g.astype(F32), adv]), adv[:1]):
        res, _ = check_all_pairs(x, qs)
        assert res[7][0] < 0  # the flat query takes its credit against these rows
    # one row alone: the bound is tight -- what is left is beta's bf16 rounding up (below 2^-7 relative), the
    # pinned coordinate's share of the error product (1 / 2d relative) and the fp32 slop
    s, c, beta, X, B, Xmin = quant_rows(adv[:1])
    slack = check_all_pairs(adv[:1], qs)[0][7][2]
    assert 0 <= slack <= float(beta[0]) * (2.0 ** -7 + 1.0 / d) + 1e-5 * float(X)
