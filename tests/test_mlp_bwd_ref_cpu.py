"""Conditions on the exact input sets of mlp_bwd_ref.py (no GPU), and the fp64
reference against torch fp64 autograd.  Statements about the inputs, not
measurements.

The sets (mlp_bwd_ref.lattice_case(n, seed 0, shift, act), one weight set for
all of them: 3 nonzeros in {-1, +1} per row, W2 row 0 / W3's SH columns / W5
rows 3..15 zero):

* n = 1, 15, 16, 17: below, at and just past one wave's 16 rows;
* n = 127, 128, 129: below, at and just past one block's 128 rows;
* n = 1029: nine blocks, the last one of 5 rows;
* n = 2 * 128 * CUs + 165 (65701 on 256 CUs): two or three passes of the
  persistent loop with a partial last block;
each with integer encodings in [-2, 2], upstream gradients in
{-1, 0, 1} x 2^(shift - 10 - e_s), e_s in 0..4 per row, one row in eight all
zero, shift in {0, -40, +30}, colour mode None or ReLU; each as all rows in
order, as a shuffled list of a third of the rows, and as a shuffled list of all
rows."""
import numpy as np
import pytest
import torch

import mlp_bwd_ref as MR
import oracle as O

SIZES = [1, 15, 16, 17, 127, 128, 129, 1029, MR.multipass_n(256)]
SHIFTS = [0, -40, 30]
ACTS = [MR.RGB_NONE, MR.RGB_RELU]


def _row_lists(n):
    return {"all": None, "list": MR.list_rows(n), "perm": MR.perm_rows(n)}


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("n", SIZES)
def test_every_gpu_set_is_exact(n, act):
    for shift in SHIFTS:
        case = MR.lattice_case(n, 0, shift, act)
        assert case.zero.any() or n < 16
        for name, rows in _row_lists(n).items():
            r = MR.check_exact(case, rows)
            print(f"n={n} act={act} shift={shift} {name}: budget 2^{r.budget_bits:.1f} of 2^24, "
                  f"block spread 2^{r.spread_bits:.1f} of 2^27")
            # (ReLU mode passes gradient only where o > 0, about one row in five: below a block's rows a
            # list may hold none -- an all-zero result is a set of its own kind)
            assert (n < 127 and act == MR.RGB_RELU) or (r.denc.any() and all(r.dW[k].any() for k in r.dW))


@pytest.mark.parametrize("act", ACTS)
def test_large_sets_put_gradient_into_every_tile(act):
    """a swapped or misplaced 16x16 tile can only show where the tiles differ: from n = 1029 on all 40 hold
    gradient (W3's SH tiles through the real SH values)"""
    for n in SIZES[-2:]:
        case = MR.lattice_case(n, 0, 0, act)
        sh = O.sh4(torch.from_numpy(case.dirs)).double().numpy()
        r = MR.mlp_bwd_ref64(case.enc, sh, case.W, case.dsig, case.drgb, act)
        assert MR.tiles_with_gradient(r.dW) == 40
        # and no two tiles of a matrix are equal
        for name, (_, od, idim) in MR.OW.items():
            t = [r.dW[name][a:a + 16, b:b + 16] for a in range(0, od, 16) for b in range(0, idim, 16)]
            assert all(not np.array_equal(t[i], t[j]) for i in range(len(t)) for j in range(i))


def test_a_shift_is_an_exact_scale():
    """the draws do not depend on the shift: the reference of shift k is 2^k x the reference of shift 0"""
    a, b = MR.lattice_case(129, 0, 0, MR.RGB_RELU), MR.lattice_case(129, 0, -40, MR.RGB_RELU)
    ra, rb = MR.check_exact(a), MR.check_exact(b)
    assert np.array_equal(np.ldexp(ra.denc, -40), rb.denc) and np.array_equal(np.ldexp(a.base, -40), b.base)
    assert all(np.array_equal(np.ldexp(ra.dW[k], -40), rb.dW[k]) for k in ra.dW)


class _Half64(torch.autograd.Function):
    """oracle._RoundHalf on fp64: fp16 storage in the forward, identity gradient"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.float16).to(torch.float64)

    @staticmethod
    def backward(ctx, g):
        return g


def _mlp_forward64(x, Ws):
    """oracle.mlp_forward's structure in fp64: ReLU hidden, fp16 at every layer output"""
    h = x
    for i, W in enumerate(Ws):
        h = _Half64.apply(h @ _Half64.apply(W).t())
        if i < len(Ws) - 1:
            h = torch.relu(h)
    return h


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("n,shift", [(17, 0), (129, -40), (1029, 30), (1029, 0)])
def test_ref64_equals_fp64_autograd(n, shift, act):
    case = MR.lattice_case(n, 0, shift, act)
    sh = O.sh4(torch.from_numpy(case.dirs)).double()
    for name, rows in _row_lists(n).items():
        ref = MR.mlp_bwd_ref64(case.enc, sh.numpy(), case.W, case.dsig, case.drgb, act, rows)
        ix = torch.from_numpy(ref.rows)
        W = {k: torch.from_numpy(v).clone().requires_grad_() for k, v in case.W.items()}
        e = torch.from_numpy(case.enc)[ix].clone().requires_grad_()
        h = _mlp_forward64(e, [W["W1"], W["W2"]])
        sig = O.TruncExpCPU.apply(h[:, 0])
        out = _mlp_forward64(torch.cat([sh[ix], h], 1), [W["W3"], W["W4"], W["W5"]])
        rgb = out[:, :3] if act == MR.RGB_NONE else torch.relu(out[:, :3])
        ((sig * torch.from_numpy(case.dsig)[ix]).sum() + (rgb * torch.from_numpy(case.drgb)[ix]).sum()).backward()
        assert np.array_equal(e.grad.numpy(), ref.denc), name
        exact = ~MR.sh_columns_mask()
        got = MR.flat_grad({k: W[k].grad.numpy() for k in W})
        want = MR.flat_grad(ref.dW)
        assert np.array_equal(got[exact], want[exact]), name
        # W3's SH columns sum inexact values: the two fp64 sums agree to fp64 roundoff
        o3, od, idim = MR.OW["W3"]
        bound = (ref.termsW3 + 2) * 2.0 ** -53 * ref.absW["W3"]
        assert (np.abs(W["W3"].grad.numpy() - ref.dW["W3"]) <= bound).all(), name


def test_pair_major_and_count_are_honoured():
    case = MR.lattice_case(129, 0, 0, MR.RGB_NONE)
    sh = np.zeros((129, 16))
    a = MR.mlp_bwd_ref64(case.enc, sh, case.W, case.dsig, case.drgb, case.act)
    pm = MR.to_pair_major(case.enc, 140, fill=9.0)
    b = MR.mlp_bwd_ref64(pm, np.zeros((140, 16)), case.W, np.pad(case.dsig, (0, 11)), np.pad(case.drgb, ((0, 11), (0, 0))),
                         case.act, rows=np.arange(129), pm_stride=140)
    assert np.array_equal(a.denc, b.denc) and all(np.array_equal(a.dW[k], b.dW[k]) for k in a.dW)
    rows = MR.perm_rows(129)
    c = MR.mlp_bwd_ref64(case.enc, sh, case.W, case.dsig, case.drgb, case.act, rows, count=40)
    d = MR.mlp_bwd_ref64(case.enc, sh, case.W, case.dsig, case.drgb, case.act, rows[:40])
    assert c.denc.shape == (40, 32) and np.array_equal(c.denc, d.denc) and np.array_equal(c.denc, a.denc[rows[:40]])
