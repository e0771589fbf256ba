"""Reference for the raw-HDR colour modes of the field (NGP_RGB_*,
include/ngp_amd.h; the reference's networks.py:68-78, 152-157), composed from
the oracle's public pieces: OracleNGPField.density + sh4 + mlp_layers +
mlp_forward give the colour net's raw fp16 output row o, mlp_forward_bound its
per-element bound d (the encoding / density-net error fed in exactly as
test_field_gpu.test_field_forward_parity forms it).  A plain helper module (not
a conftest): test_hdr_cpu.py checks it, test_hdr_gpu.py holds the kernels to it.

The activation takes an explicit positive-mask argument, so a test can take
the branch decision from the device's own forward: where |o_ref| <= d the sign
of o is not determined by the storage-point model (the set A), and a one-ulp
difference there must not decide a gradient test.

    LEAKY_RELU: rgb = rh(where(mask, o, o * float32(0.01)))
    RELU:       rgb = where(mask, o, 0)
    NONE:       rgb = o
    SIGMOID:    rgb = rh(sigmoid(o))          (OracleNGPField.forward's)

mask=None: o > 0 (torch's F.leaky_relu / relu: o == 0 takes the slope branch).
"""
import functools

import numpy as np
import torch

import oracle as O
import synthetic as S

SIGMOID, NONE, LEAKY_RELU, RELU = 0, 1, 2, 3
AMBIGUOUS_CAP = 0.05  # share of colour channels allowed in A = {|o_ref| <= d}


def activate(o, mode, mask=None, rounded=True):
    """The colour activation of `mode` on the raw output o (..., 3).
    rounded=False: no fp16 storage point (the smooth fp64 composition)."""
    rh = O.rh if rounded else (lambda t: t)
    if mode == NONE:
        return o
    if mode == SIGMOID:
        return rh(torch.sigmoid(o))
    if mask is None:
        mask = o > 0
    if mode == LEAKY_RELU:
        return rh(torch.where(mask, o, o * float(np.float32(0.01))))  # (the fp32 slope in fp64 too)
    if mode == RELU:
        return torch.where(mask, o, torch.zeros_like(o))
    raise ValueError(mode)


def color_raw(f, h, d, grad16=False):
    """The colour net's raw output rows 0..2 (fp32 holding fp16 values) from
    the density features h (N,16) and directions d."""
    Ws, _ = O.mlp_layers(f.rgb_params, f.color_dims)
    return O.mlp_forward(torch.cat([O.sh4(d).float(), h], 1), Ws, grad16=grad16)[:, :3]


def forward(f, x, d, mode, mask=None, grad16=False):
    """-> sigmas (N), rgbs (N,3), o (N,3): OracleNGPField.forward with the
    colour activation of `mode`; differentiable w.r.t. f's parameters
    (grad16: the backward's fp16 gradient storage points, oracle.rg16)."""
    old = f.grad16
    f.grad16 = grad16
    try:
        sig, h = f.density(x, return_feat=True)
    finally:
        f.grad16 = old
    o = color_raw(f, h, d, grad16)
    return sig, activate(o, mode, mask), o


@torch.no_grad()
def raw_with_bound(f, x, d):
    """-> o_ref (N,3), bound (N,3), sig_ref, h_ref, enc_ref: the raw colour
    output and the bound on |o - o'| for any implementation with the same
    fp16 storage points (test_field_forward_parity's construction)."""
    table = f.xyz_params.detach()[f.n_dens:]
    enc_ref = O.hash_encode_fwd(f.spec, x, f.xyz_min, f.xyz_max, table)
    Wd, _ = O.mlp_layers(f.xyz_params.detach()[:f.n_dens], f.dens_dims)
    h_ref, hb = O.mlp_forward_bound(enc_ref, Wd)
    Wc, _ = O.mlp_layers(f.rgb_params.detach(), f.color_dims)
    cin = torch.cat([O.sh4(d).float(), h_ref], 1)
    o, lb = O.mlp_forward_bound(cin.half(), Wc, d_in=torch.cat([torch.zeros(cin.shape[0], 16), hb], 1))
    sig = O.TruncExpCPU.apply(h_ref[:, 0])
    return o[:, :3], lb[:, :3], sig, h_ref, enc_ref


def ambiguous(o_ref, bound):
    """A = {|o_ref| <= d}: channels whose sign the storage-point model leaves open."""
    return o_ref.abs() <= bound


# ------------------------------------------------------------- input sets
def oracle_field(scale=0.5, table_init=1.0, w5_gain=1.0, seed=4):
    """The oracle field and the product's flat parameter vector
    [W1 W2 | W3 W4 W5 | table]; w5_gain multiplies the colour net's output
    layer (256: |o| reaches ~100, the HDR range)."""
    f = O.OracleNGPField(scale=scale, seed=seed, table_init=table_init)
    if w5_gain != 1.0:
        with torch.no_grad():
            f.rgb_params[-16 * 64:] *= w5_gain
    nd = f.n_dens
    flat = torch.cat([f.xyz_params.detach()[:nd], f.rgb_params.detach(), f.xyz_params.detach()[nd:]])
    return f, flat


@functools.lru_cache(maxsize=None)
def points(scale, n_marched=1000, seed=0):
    """~1000 marched samples + 512 random points incl. the box corners, built
    like test_field_gpu._points (1512 rows: a partial last 16-sample block)."""
    sc = S.SyntheticScene(W=200, H=200, n_images=10, scale=scale)
    g = torch.Generator().manual_seed(seed)
    img, pix = sc.sample_batch(4096, g)
    o, d = sc.rays(img, pix)
    c = torch.zeros(1, 3)
    h = torch.ones(1, 3) * scale
    _, ht, _ = O.ray_aabb_intersect(o, d, c, h, 1)
    ht = ht[:, 0].contiguous()
    ht[(ht[:, 0] >= 0) & (ht[:, 0] < 0.01), 0] = 0.01
    noise = torch.rand(4096, generator=g)
    _, xyzs, dirs, _, _, _ = O.raymarching_train(o, d, ht, sc.bitfield, sc.cascades, scale,
                                                 0.0 if scale <= 0.5 else 1 / 256, noise, 128, 1024)
    xyzs, dirs = xyzs[:n_marched], dirs[:n_marched]
    xr = (torch.rand(512, 3, generator=g) * 2 - 1) * scale
    xr[:8] = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * scale
    dr = torch.randn(512, 3, generator=g)
    return torch.cat([xyzs, xr]).contiguous(), torch.cat([dirs, dr]).contiguous()


SMALL_N = (1, 16, 17, 64, 65, 129)
# (name, scale, table_init, w5_gain, rows): every input set of test_hdr_gpu.py.  The
# small sets are the LAST n rows of the scale-0.5 set (random points).  The table
# is initialised at 1e-4 (tcnn's) and 1e-2: at table_init 1.0 the density
# features' fp16 ulps (7e-4), propagated through |W3| |W4| |W5| (~120 x), give
# a bound the size of o itself (measured: 54-64 % of the channels in A), so
# those sets were replaced, not the cap.
CASES = [("marched+random s0.5", 0.5, 1e-4, 1.0, None), ("marched+random s16", 16.0, 1e-4, 1.0, None),
         ("table 1e-2 s0.5", 0.5, 1e-2, 1.0, None), ("HDR range s0.5", 0.5, 1e-4, 256.0, None)] + \
        [(f"n={n}", 0.5, 1e-2, 1.0, n) for n in SMALL_N]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(f, flat, x, d, o_ref, bound, A, sig_ref, h_ref, enc_ref) of an input set."""
    _, scale, table_init, gain, rows = next(c for c in CASES if c[0] == name)
    f, flat = oracle_field(scale, table_init, gain)
    x, d = points(scale)
    if rows is not None:
        x, d = x[-rows:].contiguous(), d[-rows:].contiguous()
    o_ref, bound, sig_ref, h_ref, enc_ref = raw_with_bound(f, x, d)
    return dict(f=f, flat=flat, x=x, d=d, scale=scale, o_ref=o_ref, bound=bound, A=ambiguous(o_ref, bound),
                sig_ref=sig_ref, h_ref=h_ref, enc_ref=enc_ref)
