"""The conditions of tests/attention_cases.py, checked on its float64 / float32 CPU references alone (no GPU): the regime bands,
finiteness of every reference tensor, `winner_at` leaves the float64 result unchanged, `ties` gives weights of 1 / deg, single
in-edges weigh exactly 1, and the K1 backward reference counts at most 1e-4 of its (edge, channel) pairs as sign ties."""
import pytest
import torch as th

from tests import attention_cases as AC


@pytest.mark.parametrize("variant", AC.K1_FORWARD_VARIANTS, ids=AC.variant_id)
def test_k1_cases_sit_in_their_regime_and_have_finite_references(variant):
    """The builder asserts band and finiteness itself; here also the bands of the issue's table on both relations, the offset's
    common term, and that a saturated score would overflow an unshifted float32 exponential (the cases can tell)."""
    regime, structure, pos = variant
    for P in ((8, 16) if structure == "winner_at" else (8,)):
        for c in AC.k1_forward_pair(variant, P):
            lo, hi = AC.BANDS[regime]
            assert lo <= c.stats["median_spread"] <= hi, (c.name, c.stats)
            for t in (c.out64, c.e64, c.a64, c.out32, c.a32):
                assert bool(th.isfinite(t).all()), c.name
            if structure == "offset":
                assert AC.OFFSET_BAND[0] <= c.stats["median_common"] <= AC.OFFSET_BAND[1], (c.name, c.stats)
                assert c.stats["max_abs"] > 89.0, "an unshifted float32 exponential of these scores does not overflow"
            if regime == "saturated":
                assert c.stats["median_top"] >= AC.SATURATED_MIN_TOP, (c.name, c.stats)


def test_k1_isolated_destinations_under_saturated_scores():
    seen, _ = AC.k1_forward_pair(("saturated", None, None), 8, dist="env", seed=12)
    assert int((seen.deg == 0).sum()) > seen.N // 2 and seen.stats["n"] >= 8


@pytest.mark.parametrize("pos", AC.WINNER_POSITIONS)
@pytest.mark.parametrize("P", [8, 16])
def test_k1_winner_at_moves_the_winner_and_leaves_float64_unchanged(P, pos):
    seen, near = AC.k1_forward_pair(("saturated", "winner_at", pos), P)
    assert seen.moved > 100 and near.moved == 0          # `near` has 7 in-edges per destination: below every pass width
    assert float((seen.out64 - seen.base_out64).abs().max()) <= 1e-12 * max(1.0, float(seen.base_out64.abs().max()))
    for v in range(seen.N):
        lo, hi = int(seen.off[v]), int(seen.off[v + 1])
        if hi - lo > P:
            assert int(th.argmax(seen.e64[lo:hi, v % AC.NH])) == AC._winner_target(hi - lo, P, pos), (v, pos)


def test_k1_ties_and_single_in_edges():
    for c in AC.k1_forward_pair(("saturated", "ties", None), 8):
        n_all = n_two = 0
        for v in range(c.N):
            lo, hi = int(c.off[v]), int(c.off[v + 1])
            if c.kind[v] == 0:
                assert float((c.a64[lo:hi] - 1.0 / (hi - lo)).abs().max()) <= 1e-15, (c.name, v)
                assert float((c.a32[lo:hi].double() - 1.0 / (hi - lo)).abs().max()) <= 2e-7 / (hi - lo), (c.name, v)
                n_all += 1
            elif c.kind[v] == 1:
                top = th.topk(c.a64[lo:hi, 0], 2).values
                assert float(top[0]) == float(top[1]), (c.name, v)
                n_two += 1
        assert n_all >= 40 and n_two >= 40, (c.name, n_all, n_two)
    for c in AC.k1_forward_pair(("saturated", "deg1", None), 8):
        one = th.nonzero(c.deg == 1).flatten()
        assert one.numel() >= 80
        assert bool((c.a64[c.off[one].long()] == 1.0).all()) and bool((c.a32[c.off[one].long()] == 1.0).all())


@pytest.mark.parametrize("kind", AC.K1_BACKWARD_KINDS)
@pytest.mark.parametrize("variant", AC.K1_BACKWARD_VARIANTS, ids=lambda v: AC.variant_id(v + (None,)))
def test_k1_backward_cases_regime_dispatch_class_and_tie_cap(kind, variant):
    c = AC.k1_backward_case(kind, variant)
    if kind == "generic-sparse":
        assert c.E < 16 * c.N
    elif kind == "generic-dense":
        assert c.E >= 16 * c.N
    elif kind == "pair":
        assert c.x_src.shape[1] == 2 and 0 < c.E <= 8 * c.N and c.N % 2 == 1
    else:
        assert c.x_src.shape[1] == 4 and c.N == 300 and int(c.deg.min()) >= 16 and int(c.deg.max()) <= 128 and c.E >= 16 * c.N
    mask = c.out32 > 0
    for dtype in (th.float64, th.float32):
        for t in AC.k1_grads(c, c.d_out, mask, dtype):
            assert bool(th.isfinite(t).all()), c.name
    share = AC.k1_tie_share(c)
    assert share <= AC.TIE_CAP, f"{c.name}: {share:.2e} of the (edge, channel) pairs count as sign ties"


def test_k1_closed_form_by_degree_class_equals_autograd():
    """The shared closed form (tests/k1_closed_form.py), summed over the degree classes of a ragged relation, is the float64 autograd
    gradient of the restatement when it is handed the float64 weights - to 1e-7 of max|ref|: the two sum the cancelling terms
    de attn lrelu'(z) (attn is ~100 x its initial size here) in different orders; a wrong term would show at order one."""
    from tests.k1_closed_form import float64_closed_form_ragged
    c = AC.k1_backward_case("generic-sparse", ("peaked", None))
    mask = c.out64 > 0
    ref = AC.k1_grads(c, c.d_out, mask, th.float64)
    data = dict(x_src=c.x_src, x_dst=c.x_dst, out=c.out64, d_out=c.d_out, a_save=c.a64, prm=AC.prm_list(c.p), N=c.N)
    got, tie = float64_closed_form_ragged(data, c.off)
    for a, b, t in zip(got, ref, tie):
        assert float((a - b).abs().max()) <= 1e-7 * float(b.abs().max())
        assert bool((t >= 0).all())


def _k3_all():
    out = [("dst", sh, v) for sh in AC.K3_DST_SHAPES for v in AC.k3_dst_variants(sh)]
    return out + [("env", i, v) for i in range(len(AC.K3_ENV_SHAPES)) for v in AC.K3_ENV_VARIANTS]


@pytest.mark.parametrize("kernel,shape,variant", _k3_all(), ids=lambda x: AC.variant_id(x) if isinstance(x, tuple) and len(x) == 3 else None)
def test_k3_cases(kernel, shape, variant):
    """Every K3b case of the GPU tests: built (band, finiteness: the builder's own assertions), and its structure is what it says."""
    regime, structure, pos = variant
    c = AC.k3_dst_case(shape, variant) if kernel == "dst" else AC.k3_env_case(shape, variant)
    lo, hi = AC.BANDS[regime]
    assert lo <= c.stats["median_spread"] <= hi
    if structure == "winner_at":
        assert c.moved > 0
        assert float((c.c64 - c.base_c64).abs().max()) <= 1e-12 * max(1.0, float(c.base_c64.abs().max()))
    if structure == "ties":
        for u in th.nonzero(c.kind == 0).flatten().tolist():
            lo_, hi_ = int(c.off[u]), int(c.off[u + 1])
            assert float((c.a64[lo_:hi_] - 1.0 / (hi_ - lo_)).abs().max()) <= 1e-15
        assert int((c.kind == 0).sum()) >= 1 and int((c.kind == 1).sum()) >= 1
    if structure == "deg1":
        one = th.nonzero(c.deg == 1).flatten()
        assert one.numel() >= 1 and bool((c.a64[c.off[one].long()] == 1.0).all()) and bool((c.a32[c.off[one].long()] == 1.0).all())


@pytest.mark.parametrize("regime", ["peaked", "saturated"])
def test_disc_tarmac_cases(regime):
    d = AC.disc_case(regime)
    assert d.stats["min_margin"] >= AC.DISC_MIN_MARGIN
    for M, K, Hh in ((64, 16, 256), (72, 14, 64)):
        t = AC.tarmac_case(regime, M, K, Hh)
        lo, hi = AC.BANDS[regime]
        assert lo <= t.stats["median_spread"] <= hi


def test_agent_case_is_peaked_in_all_three_softmaxes():
    a = AC.agent_case("peaked")
    for s in a.stats:
        assert AC.BANDS["peaked"][0] <= s["median_spread"] <= AC.BANDS["peaked"][1], s
