"""Generate tests/golden/sh_probe.npz: the REFERENCE's own SH9 / probe-ray
helpers (insert/insert_utils.py get_sphere_rays, get_cubemap_rays,
get_SH_coeff, get_SH_val; imported from the reference checkout, never copied)
run on seeded inputs -- the fixture tests/test_probes_cpu.py holds
ar-nerf_amd/probes.py to.  Only arrays are recorded.

Recorded (all fp32, CPU):
  dirs        (2,65,3)  get_sphere_rays(2, 65) under torch.manual_seed(SEED)
  rgb         (2,65,3)  uniform [0,1)
  trans       (2,65,1)  uniform [0,1)  (a one-channel quantity, as 1 - opacity)
  shec        (9,3)     uniform [-1,1), DC term of channel 1 forced negative
  coeff       (2,9,3)   get_SH_coeff(dirs, rgb)
  coeff_trans (2,9,1)   get_SH_coeff(dirs, trans)
  val         (130,3)   get_SH_val(shec, dirs.reshape(-1,3))
  val_clamp   (130,3)   get_SH_val(..., clamp_postive=True)
  cube        (1,96,3)  get_cubemap_rays(1, 4)
  cube_raw    (6,4,4,3) get_cubemap_rays(1, 4, keep_raw_dim=True)
  seed        ()        SEED

Modules insert_utils imports but this container lacks (open3d, cv2) are
stubbed with empty modules: none of the recorded functions touches them.

Run:  python tests/golden/make_sh_golden.py   (needs the reference; seconds)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AR_NERF_REFERENCE", "/root/reference")
SEED = 20

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _reference_insert_utils():
    for name in ("open3d", "cv2"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, os.path.join(REF, "insert"))
    import insert_utils
    return insert_utils


def main():
    U = _reference_insert_utils()
    torch.manual_seed(SEED)
    dirs = U.get_sphere_rays(2, 65)
    g = torch.Generator().manual_seed(SEED + 1)
    rgb = torch.rand(2, 65, 3, generator=g)
    trans = torch.rand(2, 65, 1, generator=g)
    shec = torch.rand(9, 3, generator=g) * 2 - 1
    shec[0, 1] = -abs(shec[0, 1]) - 0.5
    flat = dirs.reshape(-1, 3)
    out = {
        "dirs": dirs, "rgb": rgb, "trans": trans, "shec": shec,
        "coeff": U.get_SH_coeff(dirs, rgb), "coeff_trans": U.get_SH_coeff(dirs, trans),
        "val": U.get_SH_val(shec, flat), "val_clamp": U.get_SH_val(shec, flat, clamp_postive=True),
        "cube": U.get_cubemap_rays(1, 4), "cube_raw": U.get_cubemap_rays(1, 4, keep_raw_dim=True),
    }
    arrays = {k: np.ascontiguousarray(v.numpy(), dtype=np.float32) for k, v in out.items()}
    assert (arrays["val"] < 0).any() and (arrays["val_clamp"] >= 0).all()
    arrays["seed"] = np.int64(SEED)
    path = os.path.join(HERE, "sh_probe.npz")
    np.savez(path, **arrays)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
