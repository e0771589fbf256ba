"""The C-ABI library loads on a GPU-less host and exports every entry point
include/ngp_amd.h declares; argument checks fail loudly like the
reference's CHECK_INPUT (no compute is launched here)."""
import ctypes
import os
import re

import pytest
import torch

import hashgrid as HG
import oracle as O
import vren

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    hdr = open(os.path.join(ROOT, "include", "ngp_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(ngp_[a-z0-9_]+)\s*\(", hdr)))


def test_header_declares_the_vren_surface():
    names = _declared()
    for n in ("ngp_ray_aabb_intersect", "ngp_morton3d", "ngp_morton3d_invert", "ngp_packbits",
              "ngp_march_train_count", "ngp_march_train_write", "ngp_march_test", "ngp_composite_train_fw",
              "ngp_composite_train_bw", "ngp_composite_test_fw", "ngp_field_forward", "ngp_field_backward"):
        assert n in names


def test_library_exports_every_declared_symbol():
    L = vren.lib()
    missing = [n for n in _declared() if not hasattr(L, n)]
    assert not missing, missing
    assert L.ngp_version().startswith(b"ngp_amd")


def test_every_declared_function_has_a_ctypes_signature():
    """An undeclared argtypes list lets ctypes pass Python ints as 32-bit C ints
    and floats not at all: every C-ABI entry point must be declared."""
    import hashgrid as HG
    L = HG._lib()
    missing = [n for n in _declared() if n != "ngp_version" and getattr(L, n).argtypes is None]
    assert not missing, missing


def test_library_levels_equal_oracle_levels():
    for scale in (0.5, 16.0):
        g = HG.HashGrid(scale)
        spec = O.HashGridSpec(16, 19, 16, scale=scale)
        assert g.resolutions == spec.res.tolist() and g.offsets == spec.offsets.tolist()
        assert list(g.desc.scales)[:16] == spec.scales.tolist()


def test_cpu_tensors_are_rejected_like_check_input():
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="rays_o must be a CUDA tensor"):
        vren.ray_aabb_intersect(x, x, torch.zeros(1, 3), torch.ones(1, 3), 1)
    with pytest.raises(RuntimeError, match="coords must be a CUDA tensor"):
        vren.morton3D(x.int())


def test_bad_arguments_return_einval():
    L = vren.lib()
    # null pointers with a non-zero size: rejected before any launch
    assert L.ngp_morton3d(None, 10, None, None) == -1
    assert L.ngp_composite_train_fw(None, None, None, None, None, 5, 1e-4, None, None, None, None, None, None) == -1
    assert L.ngp_march_test(None, None, None, None, 1, None, 1, 128, 0.5, 0.0, 1, 1024, None, None, None, None, None,
                            None, None) == -1
    assert L.ngp_bitfield_summary(None, 256, 128, None, None) == -1
    # zero-size calls are no-ops
    assert L.ngp_morton3d(None, 0, None, None) == 0


def test_new_entry_points_reject_bad_arguments_without_launching():
    """Argument checks run before any launch (no GPU needed): NGP_EINVAL (-1)."""
    import ctypes as C
    L = HG._lib()
    assert L.ngp_render_test_capacity(-1, 1) == -1 and L.ngp_render_test_capacity(10, 4) == 40
    assert L.ngp_render_test_begin(-1, None, None, None, None, None, None) == -1
    assert L.ngp_render_test_begin(4, None, None, None, None, None, None) == -1
    assert L.ngp_render_test_composite(None, None, None, None, None, 4, 2, None, None, None, C.c_float(1e-4),
                                       None, None, None, None) == -1
    assert L.ngp_render_test_finish(None, 4, None, None, None) == -1
    assert L.ngp_distortion_loss_fw(None, None, None, None, -1, None, None, None, None) == -1
    assert L.ngp_distortion_loss_fw(None, None, None, None, 3, None, None, None, None) == -1
    assert L.ngp_distortion_loss_bw(None, None, None, None, None, None, None, 3, None, None) == -1
    assert L.ngp_distortion_loss_fw(None, None, None, None, 0, None, None, None, None) == 0  # empty: no-op
    g = HG.HashGrid(0.5)
    assert L.ngp_density_input_grad(None, 5, C.byref(g.desc), None, None, None, None, None) == -1


def test_raw_generator_entry_point_checks_arguments_without_launching():
    """ngp_philox4x32: a negative count or a null pointer is NGP_EINVAL (-1)
    before any launch, no rows are a no-op."""
    import ctypes as C
    L = HG._lib()
    p = C.c_void_p(256)  # never dereferenced: every call below fails its checks first (or has nothing to do)
    assert L.ngp_philox4x32(p, p, -1, p, None) == -1
    assert L.ngp_philox4x32(None, p, 4, p, None) == -1
    assert L.ngp_philox4x32(p, None, 4, p, None) == -1
    assert L.ngp_philox4x32(p, p, 4, None, None) == -1
    assert L.ngp_philox4x32(None, None, 0, None, None) == 0 and L.ngp_philox4x32(p, p, 0, p, None) == 0
    assert capi.FUNCS["ngp_philox4x32"] == (c_int, [_u32p, _u32p, c_int64, _u32p, _vp])


def test_gradient_replica_entry_points_check_arguments_without_launching():
    """ngp_hash_backward_levels_rep / ngp_hash_backward_rep_floats /
    ngp_adam_step_dev_rep: sizes and
    argument checks on the host, before any launch (NGP_EINVAL = -1)."""
    import ctypes as C
    L = HG._lib()
    g = HG.HashGrid(0.5)
    d = C.byref(g.desc)
    assert L.ngp_hash_backward_rep_floats(d, 4, 8) == 8 * 2 * g.offsets[4]
    assert L.ngp_hash_backward_rep_floats(d, 0, 8) == 0
    assert L.ngp_hash_backward_rep_floats(d, 17, 8) == 0 and L.ngp_hash_backward_rep_floats(d, 4, 0) == 0
    p = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    # replicas beyond the atomic levels, replica count 0 / > 64, negative n
    assert L.ngp_hash_backward_levels_rep(p, 10, None, None, d, p, p, 0, 8, p, 9, 8, 1, None) == -1
    assert L.ngp_hash_backward_levels_rep(p, 10, None, None, d, p, p, 0, 8, p, 4, 0, 1, None) == -1
    assert L.ngp_hash_backward_levels_rep(p, 10, None, None, d, p, p, 0, 8, p, 4, 65, 1, None) == -1
    assert L.ngp_hash_backward_levels_rep(p, -1, None, None, d, p, p, 0, 8, p, 4, 8, 1, None) == -1
    f = C.c_float
    # replica range not a multiple of 4, past the Adam range, misaligned replicas
    assert L.ngp_adam_step_dev_rep(p, p, p, p, p, 64, p, f(0.9), f(0.999), f(1e-15), p, f(1.0), 1, p, 2, 8, 8,
                                   None) == -1
    assert L.ngp_adam_step_dev_rep(p, p, p, p, p, 64, p, f(0.9), f(0.999), f(1e-15), p, f(1.0), 1, p, 0, 68, 8,
                                   None) == -1
    assert L.ngp_adam_step_dev_rep(p, p, p, p, p, 64, p, f(0.9), f(0.999), f(1e-15), p, f(1.0), 1, C.c_void_p(20),
                                   0, 8, 8, None) == -1



def test_row_forward_entry_points_check_arguments_without_launching():
    """ngp_field_forward_first / ngp_rays_nonempty
    (round 4): argument checks on the host, before any launch (NGP_EINVAL =
    -1); zero rows are a no-op."""
    import ctypes as C
    L, Lv = HG._lib(), vren.lib()
    g = HG.HashGrid(0.5)
    d = C.byref(g.desc)
    p = C.c_void_p(256)  # never dereferenced: every call below fails its checks first (or has nothing to do)
    f = C.c_float(1e-4)
    # neither the counts nor the round-2 list asked for; the list without its length; a misaligned length
    assert L.ngp_field_forward_first(p, p, p, p, None, None, 8, 64, f, d, p, p, p, p, p, None, None, None, None,
                                     None) == -1
    assert L.ngp_field_forward_first(p, p, p, p, None, None, 8, 64, f, d, p, p, p, p, p, None, p, None, None,
                                     None) == -1
    assert L.ngp_field_forward_first(p, p, p, p, None, None, 8, 64, f, d, p, p, p, p, p, None, p, C.c_void_p(260),
                                     None, None) == -1
    assert L.ngp_field_forward_first(None, None, None, None, None, None, -1, 64, f, d, None, None, None, None, None,
                                     None, None, None, None, None) == -1
    assert L.ngp_field_forward_first(None, None, None, None, None, None, 0, 64, f, d, None, None, None, None, None,
                                     None, None, None, None, None) == 0
    assert Lv.ngp_rays_nonempty(p, 8, None, p, None, None, None) == -1
    assert Lv.ngp_rays_nonempty(p, -1, p, p, None, None, None) == -1
    assert Lv.ngp_rays_nonempty(p, 8, p, None, None, None, None) == -1


# ------------------------------------------------ the header as the one description (capi.py)
import subprocess  # noqa: E402
import sys  # noqa: E402
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint32, c_uint64,  # noqa: E402
                    c_ulonglong, c_void_p)

import capi  # noqa: E402
import ktimer  # noqa: E402
import renderer  # noqa: E402
import trainer  # noqa: E402

_vp, _P = capi.POINTER_TO["void"], POINTER(capi.ngp_hashgrid_t)
_fp, _i64p, _i32p, _u32p = (capi.POINTER_TO[t] for t in ("float", "int64_t", "int32_t", "uint32_t"))
# one function of each kind, read off include/ngp_amd.h by hand (pointers keep their pointee type)
_BY_HAND = {
    "ngp_morton3d": (c_int, [_i32p, c_int64, _i32p, _vp]),
    "ngp_timing_tick_ns": (c_double, []),
    "ngp_version": (c_char_p, []),
    "ngp_hash_backward_rep_floats": (c_size_t, [_P, c_int, c_int]),
    "ngp_hashgrid_levels": (c_uint32, [c_int, c_int, c_int, c_float, _fp, _u32p, _u32p, _u32p]),
    "ngp_render_test_capacity": (c_int64, [c_int64, c_int]),
    "ngp_guard_hits": (c_ulonglong, []),
    "ngp_sample_batch": (c_int, [c_uint64, c_uint64, c_int64, _vp, c_int, c_int64, c_int64, _fp, _fp, c_int64, _fp, _fp,
                                 c_float, _i64p, _i64p, _fp, _fp, _fp, _fp, _fp, _vp]),
}


@pytest.mark.parametrize("name", sorted(_BY_HAND))
def test_signature_from_header_equals_the_hand_written_one(name):
    restype, argtypes = capi.FUNCS[name]
    assert restype is _BY_HAND[name][0]
    assert len(argtypes) == len(_BY_HAND[name][1])
    assert all(a is b for a, b in zip(argtypes, _BY_HAND[name][1])), argtypes


def test_every_function_token_of_the_header_is_in_funcs():
    assert set(_declared()) == set(capi.FUNCS)


def test_declare_sets_the_header_signatures_on_the_library():
    L = vren.lib()
    for name, (restype, argtypes) in capi.FUNCS.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def _header(tmp_path, text):
    p = tmp_path / "h.h"
    p.write_text(text)
    return str(p)


def test_unmapped_type_raises_and_names_the_function(tmp_path):
    with pytest.raises(TypeError, match="ngp_takes_long"):
        capi.parse(_header(tmp_path, "int ngp_fine(int a, void* s);\nint ngp_takes_long(float* p, long n, void* s);\n"))
    with pytest.raises(TypeError, match="ngp_returns_long"):
        capi.parse(_header(tmp_path, "long ngp_returns_long(void);\n"))


def test_declaration_over_three_lines_with_comments_between_parameters_parses(tmp_path):
    funcs, _ = capi.parse(_header(tmp_path, """
/* ngp_in_a_comment(int x) is no declaration */
size_t ngp_split(const float* xyzs, /* (n,3) f32 */ int64_t n,
                 const ngp_hashgrid_t* grid,   /* the level table */
                 float scale, /* > 0 */ unsigned long long seed, void* stream);
"""))
    assert list(funcs) == ["ngp_split"]
    restype, argtypes = funcs["ngp_split"]
    assert restype is c_size_t
    assert argtypes == [_fp, c_int64, _P, c_float, c_ulonglong, _vp]


def test_a_declaration_the_parser_cannot_read_raises(tmp_path):
    with pytest.raises(TypeError, match="ngp_callback"):
        capi.parse(_header(tmp_path, "int ngp_callback(void (*fn)(int), void* stream);\n"))


def test_defines_and_enums_give_the_right_integers(tmp_path):
    _, consts = capi.parse(_header(tmp_path, """
#define NGP_GUARD_H
#define NGP_X (-3)
#define NGP_Y 0x20   /* hex */
enum { NGP_A = 0, NGP_B, /* gap */ NGP_C = 7, NGP_D,
       NGP_N };
"""))
    assert consts == {"NGP_X": -3, "NGP_Y": 32, "NGP_A": 0, "NGP_B": 1, "NGP_C": 7, "NGP_D": 8, "NGP_N": 9}


def test_python_names_keep_the_values_they_had_as_literals():
    import mlp_bwd_ref
    import render_ref
    assert (trainer.STAT_STRIPES, trainer.STAT_STRIDE) == (32, 16)
    assert (HG.RGB_SIGMOID, HG.RGB_NONE, HG.RGB_LEAKY_RELU, HG.RGB_RELU) == (0, 1, 2, 3)
    assert HG.MLP_PARAMS == 10240 and HG.N_LEVELS == 16
    assert renderer.STATE_WORDS == 8 and render_ref.STATE_WORDS == 8
    assert ktimer.ProbeTimer.WAVES == 65536
    assert (mlp_bwd_ref.RGB_NONE, mlp_bwd_ref.RGB_RELU) == (1, 3)
    assert (capi.C["NGP_OK"], capi.C["NGP_EINVAL"], capi.C["NGP_ERANGE"]) == (0, -1, -2)


def test_ktimer_name_lists_have_the_enum_lengths():
    assert len(ktimer.NAMES) == capi.C["NGP_K_COUNT"]
    assert len(ktimer.PROBES) == capi.C["NGP_P_COUNT"]


def test_hashgrid_structure_equals_the_header_typedef():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngp_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*ngp_hashgrid_t\s*;", hdr, flags=re.S).group(1)
    ctype = {"int": c_int, "float": c_float, "uint32_t": c_uint32}
    want = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        base, rest = stmt.split(None, 1)
        for d in rest.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\w+)\s*(?:\+\s*(\d+))?\s*\])?\s*", d)
            name, dim, plus = m.groups()
            if dim is not None:
                dim = (int(dim) if dim.isdigit() else capi.C[dim]) + int(plus or 0)
            want.append((name, ctype[base], dim))
    got = [(n, t._type_, t._length_) if issubclass(t, ctypes.Array) else (n, t, None)
           for n, t in capi.ngp_hashgrid_t._fields_]
    assert got == want
    assert [n for n, _, _ in got] == ["n_levels", "scales", "res", "offsets", "sizes", "xyz_min", "xyz_max"]
    assert ctypes.sizeof(capi.ngp_hashgrid_t) == 288
    assert HG.ngp_hashgrid_t is capi.ngp_hashgrid_t


def test_vren_alone_declares_the_field_entry_points():
    """vren.lib() in a process that never imports hashgrid: the field kernels'
    signatures are set all the same (one loader, one table)."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import vren; L = vren.lib(); "
            "assert 'hashgrid' not in sys.modules; "
            "assert L.ngp_field_forward.argtypes is not None; "
            "assert L.ngp_hash_binned_apply_adam.argtypes is not None")
    r = subprocess.run([sys.executable, "-c", code, os.path.dirname(os.path.abspath(vren.__file__))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------ typed pointer parameters, the checked view
_POINTEES = ("float", "int64_t", "int32_t", "uint8_t", "uint32_t", "uint64_t", "void")


def test_pointer_parameter_classes_tally_with_the_header():
    """Pointer parameters per pointee type, counted from the header text with a
    regex of this test's own, against the parameter classes in capi.FUNCS."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ngp_amd.h")).read(), flags=re.S)
    hdr = re.sub(r"^[ \t]*#.*$", "", hdr, flags=re.M)
    want = dict.fromkeys(_POINTEES, 0)
    for params in re.findall(r"\bngp_\w+\s*\(([^()]*)\)\s*;", hdr):
        for base in re.findall(r"(?:const\s+)?(\w+)\s*\*", params):
            if base not in ("ngp_hashgrid_t", "char"):
                want[base] += 1
    got = dict.fromkeys(_POINTEES, 0)
    for _, argtypes in capi.FUNCS.values():
        for a in argtypes:
            for base, cls in capi.POINTER_TO.items():
                if a is cls:
                    got[base] += 1
    assert got == want and sum(want.values()) > 600 and all(want.values()), (got, want)
    assert set(capi.POINTER_TO) == set(_POINTEES)


# (function, pointee, position of one such parameter), read off the header by hand
_TYPED = [("ngp_packbits", "float", 0), ("ngp_raygen_aabb", "int64_t", 2), ("ngp_morton3d", "int32_t", 0),
          ("ngp_bitfield_summary", "uint8_t", 0)]
_DT = {"float": (torch.float32, torch.int64), "int64_t": (torch.int64, torch.int32),  # pointee: (its dtype, a wrong one)
       "int32_t": (torch.int32, torch.int64), "uint8_t": (torch.uint8, torch.float32)}


@pytest.mark.parametrize("name,pointee,pos", _TYPED)
@pytest.mark.parametrize("view", ["raw", "checked"])
def test_typed_pointer_checks_dtype_then_contiguity_then_device(view, name, pointee, pos):
    """Each raises ctypes.ArgumentError before the C function is entered (no
    status comes back), and the order of the three checks is pinned: a CPU
    tensor of the wrong dtype fails on the dtype, a strided one of the right
    dtype on contiguity, a contiguous one on the device."""
    fn = getattr(vren.lib() if view == "raw" else vren.kernels(), name)
    assert capi.FUNCS[name][1][pos] is capi.POINTER_TO[pointee]
    right, wrong = _DT[pointee]
    args = [None] * len(capi.FUNCS[name][1])
    for i, a in enumerate(capi.FUNCS[name][1]):
        if a in (ctypes.c_int, ctypes.c_int64):
            args[i] = 0
        elif a is ctypes.c_float:
            args[i] = 0.0

    def call(t):
        a = list(args)
        a[pos] = t
        with pytest.raises(ctypes.ArgumentError) as e:
            fn(*a)
        assert f"argument {pos + 1}" in str(e.value)
        return str(e.value)

    msg = call(torch.zeros(8, dtype=wrong))
    assert str(right) in msg and str(wrong) in msg
    msg = call(torch.zeros(8, dtype=right)[::2])
    assert "contiguous" in msg and str(right) not in msg
    msg = call(torch.zeros(8, dtype=right))
    assert "CUDA" in msg and "contiguous" not in msg and str(right) not in msg


def test_void_pointer_takes_any_dtype_as_far_as_the_device_check():
    L = vren.lib()
    pos = 4  # ngp_sample_batch_dev's `const void* gt`
    assert capi.FUNCS["ngp_sample_batch_dev"][1][pos] is capi.POINTER_TO["void"]
    for dt in (torch.float16, torch.int32, torch.float64):
        a = [0, None, 0, 0, torch.zeros(4, dtype=dt), 0, 0, 0, None, None, 0, None, None, 0.0] + [None] * 8
        with pytest.raises(ctypes.ArgumentError, match="CUDA"):
            L.ngp_sample_batch_dev(*a)
        a[pos] = torch.zeros(8, dtype=dt)[::2]
        with pytest.raises(ctypes.ArgumentError, match="contiguous"):
            L.ngp_sample_batch_dev(*a)


def test_grid_descriptor_passes_as_the_struct_or_by_reference():
    g = HG.HashGrid(0.5)
    for L in (vren.lib(), vren.kernels()):
        assert L.ngp_hash_backward_rep_floats(g.desc, 4, 8) == L.ngp_hash_backward_rep_floats(ctypes.byref(g.desc), 4, 8)
        assert L.ngp_hash_backward_rep_floats(g.desc, 4, 8) == 8 * 2 * g.offsets[4]


def test_checked_view_raises_on_a_status_and_returns_values():
    K = vren.kernels()
    with pytest.raises(vren.NGPError, match="ngp_morton3d") as e:
        K.ngp_morton3d(None, 10, None, None)
    assert e.value.status == capi.C["NGP_EINVAL"] and "status -1" in str(e.value)
    assert K.ngp_morton3d(None, 0, None, None) == 0
    # value-returning functions carry no errcheck
    assert K.ngp_render_test_capacity(-1, 1) == -1 and K.ngp_render_test_capacity(10, 4) == 40
    assert K.ngp_probe_count() == capi.C["NGP_P_COUNT"] == vren.lib().ngp_probe_count()
    assert K.ngp_version() == vren.lib().ngp_version()


def test_only_status_returns_are_checked_and_the_raw_view_is_not():
    K, L = vren.kernels(), vren.lib()
    assert K is not L and K is vren.kernels() and L is vren.lib()
    assert capi.INT_VALUES == {"ngp_probe_count"}
    for name, (restype, argtypes) in capi.FUNCS.items():
        f = getattr(K, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        checked = restype is c_int and name not in capi.INT_VALUES
        assert (f.errcheck is not None) == checked, name  # ctypes: an unset errcheck reads as None
        assert getattr(L, name).errcheck is None, name
    assert L.ngp_morton3d(None, 10, None, None) == -1  # after the checked view was built
