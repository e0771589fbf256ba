"""fp64 restatement of NGP.forward with autograd to the INPUTS (positions and
directions): the reference the input-gradient kernels (csrc/inputgrad.hip:
ngp_field_input_grad, ngp_ray_segment_sum) are held to.  A plain helper module
(not a conftest), like hash_ref.py / composite_ref.py; test_pose_cpu.py checks
it on the CPU against the oracle's forward, test_input_grad_gpu.py holds the
kernels to it.  tcnn's own input-gradient arithmetic is not available: parity
unpinned, this restatement is the specification.

What is restated (fp64 arithmetic on the forward's fp32 / fp16 values):
* corner indices from oracle.hash_corners (tcnn's grid_index);
* x01 = (x - min) / (max - min) and p = float32(float64(scale_l) float64(x01) + 0.5):
  the kernels' fp32 values (the fmaf's, except on double-rounding ties), carried
  straight-through, so the cell and the in-cell position are the forward's;
* trilinear weights as fp64 products of pos_d / 1 - pos_d, fp16 table and weights;
* the forward's fp16 storage points (encoding, every layer output, SH, the
  sigmoid) straight-through: value rounded, gradient identity (rh, oracle.rh's
  rule in fp64).  The encoding's VALUE is the oracle's bit-exact fp16 encoding;
* SH4 as a differentiable polynomial of u = d / |d|; TruncExp with its backward
  clamp (custom_functions.py:162-173); the colour modes of networks.py:152-157.
"""
import torch

import oracle as O

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
TINY = 2.0 ** -126


class _RoundHalf64(torch.autograd.Function):
    """oracle.rh in the caller's dtype: fp16 value, identity gradient."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.float16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


rh = _RoundHalf64.apply


class _TruncExp64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(x.clamp(-15, 15))


def st(value, grad_path):
    """`value` in the forward, d(grad_path) in the backward (straight-through)"""
    return value.detach() + (grad_path - grad_path.detach())


def sh4_poly(u):
    """tcnn SphericalHarmonics degree 4 of the unit vector u (n,3) -> (n,16), differentiable"""
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    o = [torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z,
         -0.48860251190291987 * x, 1.0925484305920792 * xy, -1.0925484305920792 * yz,
         0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
         0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2),
         2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1.0 - 5.0 * z2),
         0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
         1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)]
    return torch.stack(o, 1)


class FieldRef64:
    """The field of flat fp32 params [W1 | W2 | W3 | W4 | W5 | table] (hashgrid.py's layout), on the CPU."""

    def __init__(self, flat_params, scale=0.5):
        p = flat_params.detach().cpu().float()
        self.spec = O.HashGridSpec(16, 19, 16, scale=scale)
        self.mn = -torch.ones(1, 3) * scale
        self.mx = torch.ones(1, 3) * scale
        h = lambda t: t.half().double()  # noqa: E731
        self.W1, self.W2 = h(p[0:2048]).view(64, 32), h(p[2048:3072]).view(16, 64)
        self.W3, self.W4, self.W5 = h(p[3072:5120]).view(64, 32), h(p[5120:9216]).view(64, 64), h(p[9216:10240]).view(16, 64)
        self.table32 = p[10240:]
        self.table = h(self.table32).view(-1, 2)

    # ------------------------------------------------------------ encoding
    def cell(self, x32):
        """the kernels' fp32 grid positions -> idx (n,L,8) global entries, p32 (n,L,3) fp32, x01 (n,3) fp32"""
        x32 = x32.detach().float().contiguous()
        idx, _ = O.hash_corners(self.spec, x32, self.mn, self.mx)
        x01 = (x32 - self.mn) / (self.mx - self.mn)
        sc = self.spec.scales.double()[None, :, None]
        p32 = (sc * x01.double()[:, None, :] + 0.5).float()
        return idx.long(), p32, x01

    @staticmethod
    def corner_weights(pos):
        """pos (...,3) -> w (...,8) in tcnn's corner order (bit d of c: the upper corner along d)"""
        w = []
        for c in range(8):
            wc = 1.0
            for d in range(3):
                wc = wc * (pos[..., d] if (c >> d) & 1 else 1 - pos[..., d])
            w.append(wc)
        return torch.stack(w, -1)

    def encode(self, x):
        """x (n,3) fp64 (values = fp32 numbers) -> enc64 (n,32): the fp64 interpolation, differentiable in x"""
        idx, p32, x01 = self.cell(x)
        x01g = st(x01.double(), (x - self.mn.double()) / (self.mx.double() - self.mn.double()))
        sc = self.spec.scales.double()[None, :, None]
        p = st(p32.double(), sc * x01g[:, None, :] + 0.5)
        pos = p - torch.floor(p32.double())
        w = self.corner_weights(pos)  # (n,L,8)
        vals = self.table[idx]  # (n,L,8,2)
        return (w[..., None] * vals).sum(2).reshape(x.shape[0], -1)

    def enc_exact(self, x):
        return O.hash_encode_fwd(self.spec, x.detach().float().contiguous(), self.mn, self.mx, self.table32).double()

    # ------------------------------------------------------------- forward
    def density_feat(self, enc):
        h1 = torch.relu(rh(enc @ self.W1.t()))
        return rh(h1 @ self.W2.t())

    def forward(self, x, d, rgb_act=0, detail=False):
        """x, d (n,3) fp64 -> sigma (n), rgb (n,3), differentiable in both.  rgb_act: hashgrid.RGB_*
        (detail: also the intermediate h (n,16), u (n,3), sh (n,16) and o (n,3))"""
        enc = st(self.enc_exact(x), self.encode(x))
        h = self.density_feat(enc)
        sigma = _TruncExp64.apply(h[:, 0])
        u = d / d.norm(dim=1, keepdim=True)
        sh = rh(sh4_poly(u))
        h3 = torch.relu(rh(torch.cat([sh, h], 1) @ self.W3.t()))
        h4 = torch.relu(rh(h3 @ self.W4.t()))
        o = rh(h4 @ self.W5.t())[:, :3]
        if rgb_act == 0:
            rgb = rh(torch.sigmoid(o))
        elif rgb_act == 1:
            rgb = o
        elif rgb_act == 2:  # F.leaky_relu on the fp16 row: o == 0 takes the slope branch
            rgb = torch.where(o > 0, o, rh(o * float(torch.tensor(0.01, dtype=torch.float32))))
        else:
            rgb = torch.relu(o)
        if detail:
            return sigma, rgb, {"h": h, "sh": sh, "o": o, "u": u}
        return sigma, rgb

    def input_grads(self, x32, d32, dL_dsig, dL_drgb, rgb_act=0):
        """dL/dx, dL/dd (n,3) fp64 for upstream dL/dsigma (n) / dL/drgb (n,3) (None: zero)"""
        x = x32.detach().double().requires_grad_(True)
        d = d32.detach().double().requires_grad_(True)
        sig, rgb = self.forward(x, d, rgb_act)
        L = 0.0
        if dL_dsig is not None:
            L = L + (sig * dL_dsig.double()).sum()
        if dL_drgb is not None:
            L = L + (rgb * dL_drgb.double()).sum()
        gx, gd = torch.autograd.grad(L, (x, d), allow_unused=True)
        return (torch.zeros_like(x) if gx is None else gx), (torch.zeros_like(d) if gd is None else gd)

    # ------------------------------------------------- position part alone
    def position_terms(self, x32, denc):
        """The position part of ngp_field_input_grad for a given dL/d(encoding) denc (n,32) fp32:
        dL/dx_d = 1/(max_d - min_d) sum_l scale_l sum_c dw_c/dpos_d (denc[2l] t_c0 + denc[2l+1] t_c1)
        -> (sum (n,3), sum of |terms| (n,3)) in fp64 over the 16 * 8 * 2 terms per component."""
        idx, p32, _ = self.cell(x32)
        pos = p32.double() - torch.floor(p32.double())  # (n,L,3)
        vals = self.table[idx]  # (n,L,8,2)
        de = denc.detach().cpu().double().view(-1, self.spec.L, 1, 2)
        sc = self.spec.scales.double()[None, :, None, None]
        ext = (self.mx.double() - self.mn.double()).reshape(3)
        tot, mag = [], []
        for dd in range(3):
            dw = []
            for c in range(8):
                f = torch.full_like(pos[..., 0], 1.0 if (c >> dd) & 1 else -1.0)
                for d2 in range(3):
                    if d2 != dd:
                        f = f * (pos[..., d2] if (c >> d2) & 1 else 1 - pos[..., d2])
                dw.append(f)
            dw = torch.stack(dw, -1)[..., None]  # (n,L,8,1)
            terms = sc * dw * de * vals / ext[dd]  # (n,L,8,2)
            tot.append(terms.sum((1, 2, 3)))
            mag.append(terms.abs().sum((1, 2, 3)))
        return torch.stack(tot, 1), torch.stack(mag, 1)


def segment_sums64(gx, gd, ts, rays_a, n_rays):
    """fp64 per-ray sums of RayMarcher.backward and the sums of |terms| -> (do, dd, |do|, |dd|) (n_rays,3);
    the terms of dd: ts * gx and gd, separately (the kernel rounds the product and the sum)."""
    gx, ts = gx.double().cpu(), ts.double().cpu()
    gd = torch.zeros_like(gx) if gd is None else gd.double().cpu()
    do, dd = torch.zeros(n_rays, 3, dtype=torch.float64), torch.zeros(n_rays, 3, dtype=torch.float64)
    ao, ad = torch.zeros_like(do), torch.zeros_like(do)
    for ray, start, n in rays_a.cpu().tolist():
        s = slice(start, start + n)
        do[ray] = gx[s].sum(0)
        ao[ray] = gx[s].abs().sum(0)
        dd[ray] = (ts[s, None] * gx[s]).sum(0) + gd[s].sum(0)
        ad[ray] = (ts[s, None] * gx[s]).abs().sum(0) + gd[s].abs().sum(0)
    return do, dd, ao, ad


def ulp16(v):
    a = v.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)

