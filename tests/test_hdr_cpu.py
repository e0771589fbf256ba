"""Raw-HDR colour modes (rgb_act='None', use_raw_HDR; NGP_RGB_* of
include/ngp_amd.h), the parts that need no GPU: argument precedence of the
_act entry points, the NGP constructor's surface, and the soundness of the
reference the GPU tests use (tests/hdr_ref.py): its autograd against fp64
central differences, and the size of the sign-ambiguous set on every input set
of test_hdr_gpu.py."""
import ctypes

import pytest
import torch

import hashgrid as HG
import hdr_ref as H
import oracle as O


def _act_calls(L, grid, n, act):
    """Every _act entry point with null pointers, `n` samples / rows and colour mode `act`."""
    g = ctypes.byref(grid.desc) if grid is not None else None
    z = None
    return {
        "ngp_field_forward_act": L.ngp_field_forward_act(z, z, n, z, g, z, z, z, z, z, z, act, z),
        "ngp_field_encode_mlp_act": L.ngp_field_encode_mlp_act(z, z, n, z, z, g, z, z, z, z, z, z, act, z),
        "ngp_field_forward_first_pre_act": L.ngp_field_forward_first_pre_act(
            z, z, z, z, z, z, n, n, ctypes.c_float(1e-4), g, z, z, z, z, z, z, z, z, z, 0, act, z),
        "ngp_field_backward_act": L.ngp_field_backward_act(z, z, n, z, g, z, z, z, z, z, z, z, act, z),
        "ngp_field_backward_mlp_act": L.ngp_field_backward_mlp_act(z, n, z, z, z, 0, z, z, z, z, z, act, z),
    }


@pytest.mark.parametrize("n", [0, 5])
@pytest.mark.parametrize("act", [-1, 4])
def test_a_mode_outside_0_3_is_refused_before_anything_else(n, act):
    """NGP_EINVAL before any other argument is looked at: null pointers, no
    grid, n == 0 and n > 0 alike (the header's stated precedence)."""
    L = HG._lib()
    for with_grid in (False, True):
        res = _act_calls(L, HG.HashGrid(0.5) if with_grid else None, n, act)
        assert all(v == -1 for v in res.values()), res


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_every_mode_is_accepted_and_an_empty_call_launches_nothing(act):
    res = _act_calls(HG._lib(), HG.HashGrid(0.5), 0, act)
    assert all(v == 0 for v in res.values()), res


def test_mode_constants_match_the_header():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngp_amd.h")).read()
    for name, v in (("SIGMOID", 0), ("NONE", 1), ("LEAKY_RELU", 2), ("RELU", 3)):
        assert f"#define NGP_RGB_{name} {v}" in hdr
        assert getattr(HG, f"RGB_{name}") == v == getattr(H, name)


def test_ngp_constructor_surface():
    from models.networks import NGP
    hdr, ldr = NGP(0.5, 'None', True), NGP(0.5)
    assert list(hdr.state_dict().keys()) == list(ldr.state_dict().keys())  # the same checkpoint layout
    assert all(a.shape == b.shape for a, b in zip(hdr.state_dict().values(), ldr.state_dict().values()))
    assert hdr.rgb_mode() == HG.RGB_LEAKY_RELU and hdr.rgb_mode(True) == HG.RGB_RELU
    # a sigmoid model under use_raw_HDR: leaky_relu of a sigmoid is the identity
    both = NGP(0.5, 'Sigmoid', True)
    assert both.rgb_mode() == both.rgb_mode(True) == ldr.rgb_mode() == HG.RGB_SIGMOID
    with pytest.raises(NotImplementedError, match="tonemapper"):
        NGP(0.5, 'None', False)
    with pytest.raises(NotImplementedError):
        NGP(0.5, 'Tanh')
    with pytest.raises(NotImplementedError):
        NGP(0.5, 'Tanh', True)


def test_leaky_relu_formula_is_torchs_on_half():
    """The kernels' mode 2 / the helper's formula against F.leaky_relu on an
    fp16 tensor: every finite fp16 value, bit for bit."""
    o16 = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(torch.float16)
    o16 = o16[torch.isfinite(o16)]
    ref = torch.nn.functional.leaky_relu(o16)
    got = H.activate(o16.float(), H.LEAKY_RELU).half()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    # (as values: torch.relu keeps the sign of -0, the table's `o > 0 ? o : 0` gives +0)
    assert torch.equal(H.activate(o16.float(), H.RELU), torch.relu(o16).float())


def _mlp64(x, Ws):
    h = x
    for i, W in enumerate(Ws):
        h = h @ W.t()
        if i < len(Ws) - 1:
            h = torch.relu(h)
    return h


@pytest.mark.parametrize("table_init", [1.0, 1e-2])
def test_helper_autograd_matches_fp64_central_differences(table_init):
    """Directional derivatives of sum(G * rgb) along 8 seeded random weight
    directions (density and colour MLP weights; 64 points, table_init 1.0):
    the helper's autograd (fp16 storage points, straight-through) against
    central differences of the same composition in fp64 without storage
    points, at the fp16-rounded weights, the mask held fixed.  Only channels
    with |o| > 4 d carry gradient, so the kink is not crossed.  Tolerance: 4 x
    the same discrepancy measured here for the sigmoid activation (what the
    storage points cost any activation; leaky / relu add one multiplication).
    At table_init 1.0 the bound d (the density features' fp16 ulps through
    |W3| |W4| |W5|, ~120 x) is the size of o itself and a single channel of
    the 192 qualifies; the same test at table_init 1e-2 has 164, on both
    branches."""
    f, _ = H.oracle_field(0.5, table_init)
    x, d = H.points(0.5)
    x, d = x[-64:].contiguous(), d[-64:].contiguous()
    o_ref, bound, _, _, enc_ref = H.raw_with_bound(f, x, d)
    keep = o_ref.abs() > 4 * bound
    print(f"{int(keep.sum())} of {keep.numel()} channels with |o| > 4 d")
    mask = o_ref > 0
    if table_init == 1.0:
        assert int(keep.sum()) >= 1
    else:  # most channels, and both branches carry gradient
        assert int(keep.sum()) > 96 and bool((mask & keep).any()) and bool((~mask & keep).any())
    g = torch.Generator().manual_seed(21)
    G = torch.randn(64, 3, generator=g) * keep
    nd = f.n_dens
    w0 = torch.cat([O.rh(f.xyz_params.detach()[:nd]), O.rh(f.rgb_params.detach())]).double()
    dirs = [torch.randn(w0.numel(), generator=g).double() * w0.abs().mean() for _ in range(8)]
    sh = O.sh4(d).double()

    def loss64(w, mode):
        Wd, _ = O.mlp_layers(w[:nd], f.dens_dims)
        Wc, _ = O.mlp_layers(w[nd:], f.color_dims)
        h = _mlp64(enc_ref.double(), Wd)
        o = _mlp64(torch.cat([sh, h], 1), Wc)[:, :3]
        return float((H.activate(o, mode, mask, rounded=False) * G.double()).sum())

    def discrepancy(mode):
        f.zero_grad()
        _, rgb, _ = H.forward(f, x, d, mode, mask=mask)
        (rgb * G).sum().backward()
        ga = torch.cat([f.xyz_params.grad[:nd], f.rgb_params.grad]).double()
        eps = 1e-6
        fd = torch.tensor([(loss64(w0 + eps * v, mode) - loss64(w0 - eps * v, mode)) / (2 * eps) for v in dirs])
        an = torch.tensor([float(ga @ v) for v in dirs])
        # worst direction, relative to the rms derivative over the 8 (one direction's may nearly cancel)
        return float((an - fd).abs().max() / fd.pow(2).mean().sqrt())

    base = discrepancy(H.SIGMOID)
    tol = 4 * base
    print(f"sigmoid: autograd vs fp64 central differences {base:.2e} (worst of 8 directions); tolerance {tol:.2e}")
    assert 0 < base < 5e-2
    for name, mode in (("leaky_relu", H.LEAKY_RELU), ("relu", H.RELU), ("none", H.NONE)):
        e = discrepancy(mode)
        print(f"{name}: {e:.2e}")
        assert e <= tol, (name, e, tol)


@pytest.mark.parametrize("name", [c[0] for c in H.CASES])
def test_the_sign_ambiguous_set_is_small_on_every_gpu_input_set(name):
    """A = {|o_ref| <= d} holds at most 5 % of the colour channels of every
    input set test_hdr_gpu.py uses (there the branch is taken from the device's
    forward inside A, and asserted equal to the oracle's outside it)."""
    c = H.case(name)
    A = c["A"]
    share = float(A.float().mean())
    print(f"{name}: |A| = {int(A.sum())} of {A.numel()} channels ({share:.2%}); max |o_ref| "
          f"{float(c['o_ref'].abs().max()):.1f}")
    assert share <= H.AMBIGUOUS_CAP
    if "HDR" in name:
        assert float(c["o_ref"].abs().max()) > 50  # the HDR range is really reached
