"""The designed rows of tests/_knn_cases.py do what they claim, without a GPU: fp32 rows in, the bf16 round trip through
``torch.bfloat16``, float64 sums out.  The rows are unit rows; A is q's true nearest neighbour by a gap the GPU tests can
see; the bf16 scores put A below every decoy by MORE than twice the margin the screen shipped with (0.0042) and by less
than twice the bound that holds, 2**-7 + 2**-16.  And that bound itself: it holds over the designs and a few thousand
sign-flipped, permuted and rescaled variants of them, some of which exceed 0.0042."""
import pytest
import torch

import _knn_cases as K

# every width the GPU cases use (64: one K chunk, h cut short by the width; 256: h cut short; 768: the flagship width) and the
# other widths of the issue's table; k: the GPU cases' (40 decoys at D = 256 share the last two columns for their fillers)
SHAPES = [(64, 2), (128, 2), (256, 2), (256, 12), (256, 40), (768, 4), (1024, 4), (768, 64)]


def test_design_shapes_are_the_documented_ones():
    want = {64: (2.0 ** -3, 30), 128: (2.0 ** -3, 31), 256: (2.0 ** -4, 126), 768: (2.0 ** -4, 127), 1024: (2.0 ** -5, 508)}
    for D, ph in want.items():
        assert K.shape_of(D) == ph
        assert K.default_nlow(D) == (2 if D <= 128 else 10)


@pytest.mark.parametrize("D,k", SHAPES)
def test_designed_rows_defeat_the_old_margin_and_not_the_true_bound(D, k):
    """Margins reached (float64 sums of the bf16 products), old = min_j approx(B_j) - 2 * 0.0042 - approx(A), true = approx(A) - (max_j approx(B_j)
    - 2 eps_true), gap = exact(A) - exact(B_1):
        D = 64 (nlow 2)   gap 2.3e-4  old 2.2e-4  true 7.0e-3       D = 128 (nlow 2)  gap 2.3e-4  old 5.2e-4  true 6.7e-3
        D = 256           gap 3.0e-4  old 6.1e-4  true 6.7e-3       D = 768           gap 3.0e-4  old 6.8e-4  true 6.6e-3
        D = 1024          gap 6.6e-5  old 8.9e-4  true 6.4e-3
    so the 1e-4 of room asked of `old` is reached at every width, D = 64 included (nlow = 3 would leave exactly 1.0e-4
    there, nlow = 10 lets A through)."""
    d = K.build(D, k)
    rows = torch.cat([d.q[None], d.A[None], d.B])
    assert rows.dtype == torch.float32 and rows.shape == (k + 2, D)
    assert float((rows.double().norm(dim=1) - 1.0).abs().max()) <= 1e-6
    assert len({tuple(r.tolist()) for r in rows}) == k + 2                      # k + 2 distinct rows
    exact = K.exact_scores(d.q, rows)                                           # self, A, B_1 .. B_k
    assert bool((exact[:-1] >= exact[1:]).all()) and exact[0] > exact[1] > exact[2]
    assert float(exact[1] - exact[2]) >= 5e-5                                   # 25 x the 2e-6 the GPU tests allow
    approx = K.approx_scores(d.q, rows)
    a, b = float(approx[1]), approx[2:]
    assert a < float(b.min()) - 2 * K.EPS_OLD - 1e-4                            # the old margin never emits A ...
    assert a > float(b.max()) - 2 * K.EPS_TRUE                                  # ... the bound that holds keeps it
    # fp32 accumulation moves these scores by far less than the 1e-4 of room (any order: <= D 2**-24 sum |products| < 6.2e-5)
    a32 = K.bf16_round(rows).float() @ K.bf16_round(d.q).float()
    assert float((a32.double() - approx).abs().max()) <= 1e-6


def _variants(gen):
    """Unit fp32 rows derived from the designs: columns permuted, signs flipped (per column: products keep their sign;
    per element of one row: they do not), halves rescaled, and the eta of every element redrawn (which side of the bf16
    midpoint it falls on)."""
    out = []
    for D, k in ((64, 2), (128, 2), (256, 3), (768, 2), (1024, 2)):
        d = K.build(D, k)
        base = torch.cat([d.q[None], d.A[None], d.B]).double()
        out.append((D, base.float()))
        for _ in range(60):
            v = base.clone()
            kind = int(torch.randint(0, 4, (1,), generator=gen))
            if kind >= 1:   # signs: per column (shared) ...
                v = v * (torch.randint(0, 2, (1, D), generator=gen) * 2 - 1).double()
            if kind >= 2:   # ... and per element
                v = v * (torch.randint(0, 2, v.shape, generator=gen) * 2 - 1).double()
            if kind == 3:   # the side of the midpoint, element by element, and a rescaled half
                v = v * (1.0 + K.ETA * 2 * (torch.randint(0, 2, v.shape, generator=gen) * 2 - 1).double())
                v[:, : D // 2] *= float(torch.rand(1, generator=gen)) + 0.5
            v = v[:, torch.randperm(D, generator=gen)]
            v = (v / v.norm(dim=1, keepdim=True)).float()
            out.append((D, v))
    return out


def test_bf16_screen_error_bound_holds_and_is_nearly_attained():
    """|approx - exact| <= (2**-7 + 2**-16) |q| |c| for every pair of rows of every variant (elementwise |x~ - x| <= u |x|,
    u = 2**-8, hence |sum x~ y~ - sum x y| <= (2 u + u**2) sum |x| |y|), and the old 0.0042 is exceeded: not vacuous."""
    gen = torch.Generator().manual_seed(20)
    worst, pairs, over_old = 0.0, 0, 0
    for D, v in _variants(gen):
        x64, xb = v.double(), K.bf16_round(v)
        err = (xb @ xb.t() - x64 @ x64.t()).abs()
        nrm = x64.norm(dim=1)
        bound = K.EPS_TRUE * nrm[:, None] * nrm[None, :]
        assert bool((err <= bound).all()), (D, float((err / bound).max()))
        worst = max(worst, float(err.max()))
        pairs += err.numel()
        over_old += int((err > K.EPS_OLD).sum())
    assert pairs >= 3000
    assert over_old >= 1 and worst > K.EPS_OLD
    assert worst <= K.EPS_TRUE * (1 + 1e-6)
