"""The training step's forms of the exposure tonemappers (DESIGN.md §19;
ngp_sample_exposure*, ngp_tonemap_forward_rows, ngp_tonemap_backward_indexed,
ngp_unit_exposure_term) restated in NumPy on tests/tonemap_ref.py: which slots
a call owns, and the fp64 backward over a sample list with its error bars.
Shared by test_exposure_fused_cpu.py and the two GPU files."""
import functools

import numpy as np

import tonemap_ref as T

ROW_SAMPLES = (0, 1, 63, 64, 65, 200)  # a row's first chunk is one wave: its edges, and a row past it
LIST_LENGTHS = (1, 63, 64, 65, 257, 4099)  # wave, block and grid edges of the backward


def rays_case(seed=0, gap=3):
    """rays_a (R,3) i64 with rows of ROW_SAMPLES samples (each count twice) in shuffled ray order, `gap`
    unowned slots between segments and before the first -> (rays_a, n = slots in all)."""
    g = np.random.default_rng(seed)
    counts = np.array(ROW_SAMPLES * 2)
    R = len(counts)
    counts = counts[g.permutation(R)]
    rays = g.permutation(R)
    rays_a = np.zeros((R, 3), np.int64)
    pos = gap
    for r in range(R):
        rays_a[r] = (rays[r], pos, counts[r])
        pos += counts[r] + gap
    return rays_a, pos


def expand_exposure(rays_a, out, img_idxs=None, img_exposure=None, ray_exposure=None):
    """`out` (n) f32 with every row's slots [start, start + N) set to its ray's exposure (a copy)"""
    out = np.array(out, np.float32)
    for ray, start, N in np.asarray(rays_a):
        e = ray_exposure[ray] if ray_exposure is not None else img_exposure[img_idxs[ray]]
        out[start:start + N] = e
    return out


def owned(rays_a, n):
    """(n) bool: the slots some row owns"""
    m = np.zeros(n, bool)
    for _, start, N in np.asarray(rays_a):
        m[start:start + N] = True
    return m


def rows_selection(rays_a, rows, n_rows_dev, first, n):
    """(n) bool: the samples ngp_tonemap_forward_rows writes -- the first min(N_r, first) of the rows
    rows[:n_rows_dev] (rows None: every row)"""
    rays_a = np.asarray(rays_a)
    listed = np.arange(len(rays_a)) if rows is None else np.asarray(rows)
    if n_rows_dev is not None:
        listed = listed[:min(int(n_rows_dev), len(listed))]
    m = np.zeros(n, bool)
    for r in listed:
        start, N = rays_a[r, 1], rays_a[r, 2]
        m[start:start + min(N, first)] = True
    return m


def list_selection(idx, count, n):
    """The rows a sample list names: idx[:min(count, n)] without the indices outside [0, n)"""
    idx = np.asarray(idx)[:min(int(count), n)]
    return idx[(idx >= 0) & (idx < n)]


@functools.lru_cache(maxsize=None)
def list_case(length):
    """tonemap_ref.case of n = 2 length + TAIL rows and a shuffled subset of `length` of them (i32).
    From two listed rows up, the list's second row has a zero upstream gradient (the case's own zero
    rows, a tenth of all, may miss a short list), so "a listed row with a zero gradient" always exists."""
    n = 2 * length + 21
    c = dict(T.case(n))
    idx = np.random.default_rng(7000 + length).permutation(n)[:length].astype(np.int32)
    if length >= 2:
        c["dy"] = c["dy"].copy()
        c["dy"][idx[1]] = 0.0
    return c, idx


def backward_indexed(w, x, e, dy, idx, count=None):
    """tonemap_ref.backward over the rows of a list (each once): dx (n,3) f64, NaN off the list; grad,
    grad_bar (2^-23 (n_terms + 64) S + Bamb with n_terms = the list's length), dx_bar (n,3), n_amb."""
    x, e, dy = np.asarray(x), np.asarray(e), np.asarray(dy)
    n = x.shape[0]
    rows = list_selection(idx, len(idx) if count is None else count, n)
    assert len(np.unique(rows)) == len(rows)
    ref = T.backward(w, x[rows], e[rows], dy[rows])
    dx = np.full((n, 3), np.nan)
    dx_bar = np.zeros((n, 3))
    dx[rows], dx_bar[rows] = ref["dx"], ref["dx_bar"]
    return {"rows": rows, "dx": dx, "dx_bar": dx_bar, "grad": ref["grad"], "grad_bar": ref["grad_bar"],
            "n_amb": ref["n_amb"]}


def unit_exposure(w, target):
    """The unit-exposure term in fp64: (loss, grad (PARAMS), grad_bar) of mean_c 0.5 (y_c - target)^2 at
    log radiance 0, exposure 1"""
    zero = np.zeros((1, 3), np.float32)
    y = T.forward(w, zero, np.ones(1))
    ref = T.backward(w, zero, np.ones(1), ((y - target) / 3).astype(np.float32))
    return float((0.5 * (y - target) ** 2).mean()), ref["grad"], ref["grad_bar"]
