"""fp64 restatement of the fused step's pose refinement (csrc/pose.hip): the pose
composition [Rod(dR) R | t + dT] (train.py:92-95) and the chain rule from per-ray
gradients to the per-image dR / dT, written from the formulas and not from the
kernel.  Checked on the CPU (test_pose_chain_cpu.py) against the reference
function's recorded outputs and against torch.autograd of an fp64 copy of
axisangle_to_R + get_rays; the GPU tests hold the kernels to it.

Every function also returns the sum of the absolute values of the terms it adds
("mag"), weighted per term by the number of roundings the fp32 kernel spends on
that term's path where a count is asked for: the error bars of
test_pose_fused_gpu.py are u * sum_t k_t |term_t|."""
import math

import torch

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20  # second-order terms of the first-order bounds
TINY = 2.0 ** -126
GUARD = 1e-7  # the reference's theta = |v| + 1e-7


def skew(v):
    """(n,3) -> (n,3,3), the reference's skew_v"""
    z = torch.zeros_like(v[:, 0])
    return torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], 1), torch.stack([v[:, 2], z, -v[:, 0]], 1),
                        torch.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def coefficients(theta):
    """A, B, A', B' at theta > 0 (fp64).  1 - cos as 2 sin^2(theta/2): in fp64 the plain form has lost
    half its digits at theta = 1e-7 already.  A' and B' from a 12-term series below 0.5 (fp64 cancellation
    of the closed forms there: up to 1e-16 * 3 / theta^2 relative), closed forms above."""
    th = theta.double()
    s, c, sh = torch.sin(th), torch.cos(th), torch.sin(th / 2)
    A = s / th
    B = 2 * (sh / th) ** 2
    dA_c = (th * c - s) / th ** 2
    dB_c = (th * s - 4 * sh ** 2) / th ** 3
    dA_s, dB_s = torch.zeros_like(th), torch.zeros_like(th)
    for n in range(1, 13):
        dA_s = dA_s + (-1) ** n * 2 * n / math.factorial(2 * n + 1) * th ** (2 * n - 1)
        dB_s = dB_s + (-1) ** n * 2 * n / math.factorial(2 * n + 2) * th ** (2 * n - 1)
    small = th < 0.5
    return A, B, torch.where(small, dA_s, dA_c), torch.where(small, dB_s, dB_c)


def condition_numbers(theta):
    """|theta f'(theta) / f(theta)| for f = A, B, A', B': how a relative error of theta (its own roundings)
    shows in each coefficient.  Central differences in fp64 at a relative step of 1e-5 (error ~1e-10)."""
    th = theta.double()
    h = 1e-5 * th
    lo, hi, mid = coefficients(th - h), coefficients(th + h), coefficients(th)
    return tuple(((b - a) / (2 * h) * th / m).abs() for a, b, m in zip(lo, hi, mid))


def rodrigues(v):
    """(n,3) -> Rod (n,3,3), theta (n), |v| (n), all fp64"""
    v = v.double()
    nv = v.norm(dim=1)
    th = nv + GUARD
    A, B, _, _ = coefficients(th)
    K = skew(v)
    eye = torch.eye(3, dtype=torch.float64).expand(len(v), 3, 3)
    return eye + A[:, None, None] * K + B[:, None, None] * (K @ K), th, nv


def compose(poses, ext, k_terms=None):
    """poses (n,3,4), ext (>= 6n) = [dR | dT | pad] -> poses_eff (n,3,4) fp64 and mag (n,3,4):
    sum_t k_t |term_t| of every entry.  Rotation entry (a,b) = sum_c (delta_ac + A K_ac + B K2_ac) R_cb: three
    terms per c; k_terms(theta) -> (k_I, k_AK, k_BK2) (n) each, default 1.  Translation: |t| + |dT|."""
    n = poses.shape[0]
    P = poses.double()
    v = ext[:3 * n].double().view(n, 3)
    dT = ext[3 * n:6 * n].double().view(n, 3)
    rod, th, _ = rodrigues(v)
    out = torch.cat([rod @ P[:, :, :3], (P[:, :, 3] + dT)[..., None]], -1)
    A, B, _, _ = coefficients(th)
    K = skew(v)
    K2 = K @ K
    one = torch.ones(n, dtype=torch.float64)
    kI, kA, kB = (one, one, one) if k_terms is None else k_terms(th)
    eye = torch.eye(3, dtype=torch.float64).expand(n, 3, 3)
    w = (kI[:, None, None] * eye + (kA * A.abs())[:, None, None] * K.abs()
         + (kB * B.abs())[:, None, None] * K2.abs())
    mag = torch.cat([w @ P[:, :, :3].abs(), (P[:, :, 3].abs() + dT.abs())[..., None]], -1)
    return out, mag


def rod_grad(v, M):
    """dL/dv (n,3) for dL/dRod = M (n,3,3), closed form:
    dRod/dv_k = A E_k + B (E_k K + K E_k) + (A' K + B' K^2) v_k / |v|   (0 for the last term at |v| = 0).
    Also the per-(k) list of (term, coefficient index) pieces for the error bars: pieces[c] (n,3) is the sum of
    |M_ab| |coef_c| |d.../dv_k| over the entries multiplied by coefficient c in (A, B, A', B')."""
    v, M = v.double(), M.double()
    n = len(v)
    nv = v.norm(dim=1)
    th = nv + GUARD
    A, B, dA, dB = coefficients(th)
    K = skew(v)
    K2 = K @ K
    rho = torch.where(nv[:, None] > 0, v / nv.clamp_min(1e-300)[:, None], torch.zeros_like(v))
    g = torch.zeros(n, 3, dtype=torch.float64)
    pieces = [torch.zeros(n, 3, dtype=torch.float64) for _ in range(4)]
    aM = M.abs()
    for k in range(3):
        e = torch.zeros(n, 3, dtype=torch.float64)
        e[:, k] = 1
        E = skew(e)
        EK = E @ K + K @ E
        g[:, k] = ((A[:, None, None] * E + B[:, None, None] * EK
                    + (dA[:, None, None] * K + dB[:, None, None] * K2) * rho[:, k, None, None]) * M).sum((1, 2))
        # E K + K E = e v^T + v e^T - 2 v_k I entry by entry: its absolute terms
        aEK = (e[:, :, None] * v[:, None, :]).abs() + (v[:, :, None] * e[:, None, :]).abs() \
            + 2 * v[:, k].abs()[:, None, None] * torch.eye(3, dtype=torch.float64)
        aK2 = (v[:, :, None] * v[:, None, :]).abs() + (nv ** 2)[:, None, None] * torch.eye(3, dtype=torch.float64)
        pieces[0][:, k] = A.abs() * (E.abs() * aM).sum((1, 2))
        pieces[1][:, k] = B.abs() * (aEK * aM).sum((1, 2))
        pieces[2][:, k] = dA.abs() * rho[:, k].abs() * (K.abs() * aM).sum((1, 2))
        pieces[3][:, k] = dB.abs() * rho[:, k].abs() * (aK2 * aM).sum((1, 2))
    return g, pieces


def pose_grad(go, gd, img, pix, directions, poses, ext, k_coef=None, k_common=0.0):
    """The chain rule: per-ray gradients go, gd (n_rays,3), the batch (img, pix), directions (HW,3), the
    ORIGINAL poses (n_img,3,4), ext -> grad (6 n_img + pad) fp64 in ext's layout, and bound (same shape) =
    sum_t (n_i + k_common + k_coef_c(t)) |term_t|: for dL/dT_i the terms are the image's go; for dL/ddR_i the
    products gd_r[a] c_r[c] R_i[b][c] dRod[a][b]/dv_k, one coefficient c in (A, B, A', B') each.
    k_coef(theta) -> 4 tensors (n_img); None: zeros."""
    n_img = poses.shape[0]
    go, gd, P = go.double(), gd.double(), poses.double()
    c = directions.double()[pix]
    v = ext[:3 * n_img].double().view(n_img, 3)
    cnt = torch.zeros(n_img, dtype=torch.float64).index_add(0, img, torch.ones(len(img), dtype=torch.float64))
    z3 = torch.zeros(n_img, 3, dtype=torch.float64)
    dT, adT = z3.index_add(0, img, go), z3.index_add(0, img, go.abs())
    outer = gd[:, :, None] * c[:, None, :]
    z33 = torch.zeros(n_img, 3, 3, dtype=torch.float64)
    G, aG = z33.index_add(0, img, outer), z33.index_add(0, img, outer.abs())
    M = G @ P[:, :, :3].transpose(1, 2)
    aM = aG @ P[:, :, :3].abs().transpose(1, 2)
    dv, _ = rod_grad(v, M)
    _, pieces = rod_grad(v, aM)
    th = v.norm(dim=1) + GUARD
    kc = [torch.zeros(n_img, dtype=torch.float64)] * 4 if k_coef is None else k_coef(th)
    base = cnt + k_common
    bdv = sum((base + kc[i])[:, None] * pieces[i] for i in range(4))
    n_pad = (6 * n_img + 3) // 4 * 4
    grad, bound = torch.zeros(n_pad, dtype=torch.float64), torch.zeros(n_pad, dtype=torch.float64)
    grad[:3 * n_img], grad[3 * n_img:6 * n_img] = dv.reshape(-1), dT.reshape(-1)
    bound[:3 * n_img], bound[3 * n_img:6 * n_img] = bdv.reshape(-1), (base[:, None] * adT).reshape(-1)
    return grad, bound


# ---- an fp64 copy of the project's axisangle_to_R + get_rays, for torch.autograd (the CPU test's second opinion)
def axisangle_to_R64(v, literal=False):
    """datasets.ray_utils.axisangle_to_R in fp64.  literal: 1 - cos(theta) as the project writes it; else as
    2 sin^2(theta/2), the same function without the cancellation.  fp64 does not rescue the literal form where
    refinement lives: at theta = 2e-7, 1 - cos(theta) = 2e-14 is held to 1.1e-16 absolute, its quotient by
    theta^2 to 0.3 %, and autograd's sin/theta^2 - 2 (1 - cos)/theta^3 (two terms of 5e6 that differ by 2e-8) to
    ~1e4 absolute: 6.4e-11 of the pose gradient measured at |v| = 1e-7, against 1e-15 for the other form."""
    v = v.double()
    zero = torch.zeros_like(v[:, :1])
    skew_v = torch.stack([torch.cat([zero, -v[:, 2:3], v[:, 1:2]], 1), torch.cat([v[:, 2:3], zero, -v[:, 0:1]], 1),
                          torch.cat([-v[:, 1:2], v[:, 0:1], zero], 1)], dim=1)
    norm_v = (torch.norm(v, dim=1) + GUARD)[:, None, None]
    eye = torch.eye(3, dtype=torch.float64)
    one_minus_cos = 1 - torch.cos(norm_v) if literal else 2 * torch.sin(norm_v / 2) ** 2
    return eye + (torch.sin(norm_v) / norm_v) * skew_v + (one_minus_cos / norm_v ** 2) * (skew_v @ skew_v)


def rays64(ext, img, pix, directions, poses, literal=False):
    """PoseRefiner.rays in fp64: rays_o, rays_d (n_rays,3) of the batch, differentiable in ext"""
    n = poses.shape[0]
    P = poses.double()
    dR, dT = ext[:3 * n].view(n, 3), ext[3 * n:6 * n].view(n, 3)
    R = (axisangle_to_R64(dR, literal) @ P[:, :, :3])[img]
    d = directions.double()[pix]
    rays_d = d[:, None, 0] * R[..., 0] + d[:, None, 1] * R[..., 1] + d[:, None, 2] * R[..., 2]
    return (P[:, :, 3] + dT)[img], rays_d
