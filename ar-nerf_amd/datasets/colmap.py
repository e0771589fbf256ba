"""datasets/colmap.py:15-166 of the reference: COLMAP scenes (mip-NeRF 360
'garden' & co.): intrinsics from sparse/0/cameras.bin (camera 1), c2w from
images.bin sorted by image name, centred on the point cloud's average pose
(center_poses) and scaled so the closest camera is at distance 1; every 8th
image is the test set.  A root_dir containing 'HDR-NeRF' is a multi-exposure
scene (datasets/colmap.py:91-123, 141-161): its own train / test picks, the
poses repeated per exposure, and the image's exposure (the scene's table at
the last digit of the file name) as the rays' 4th channel."""
import glob
import os

import numpy as np
import torch

from .base import BaseDataset
from .color_utils import read_image
from .colmap_utils import read_cameras_binary, read_images_binary, read_points3d_binary
from .ray_utils import center_poses, create_spheric_poses, get_ray_directions


def _quarter_stops(first):
    return {e: first * 4 ** e for e in range(5)}


# exposure index (the last digit of the image's name) -> exposure, per HDR-NeRF scene
HDR_NERF_EXPOSURES = {
    **dict.fromkeys(('bathroom', 'bear', 'chair', 'desk'), _quarter_stops(1 / 8)),
    **dict.fromkeys(('diningroom', 'dog'), _quarter_stops(1 / 16)),
    'sofa': {0: 0.25, 1: 1, 2: 2, 3: 4, 4: 16},
    'sponza': {0: 0.5, 1: 2, 2: 4, 3: 8, 4: 32},
    'box': {0: 2 / 3, 1: 1 / 3, 2: 1 / 6, 3: 0.1, 4: 0.05},
    'computer': {0: 1 / 3, 1: 1 / 8, 2: 1 / 15, 3: 1 / 30, 4: 1 / 60},
    'flower': {0: 1 / 3, 1: 1 / 6, 2: 0.1, 3: 0.05, 4: 1 / 45},
    'luckycat': {0: 2, 1: 1, 2: 0.5, 3: 0.25, 4: 0.125},
}


class ColmapDataset(BaseDataset):
    def __init__(self, root_dir, split='train', downsample=1.0, **kwargs):
        super().__init__(root_dir, split, downsample)
        self.read_intrinsics()
        if kwargs.get('read_meta', True):
            self.read_meta(split, **kwargs)

    def read_intrinsics(self):
        cam = read_cameras_binary(os.path.join(self.root_dir, 'sparse/0/cameras.bin'))[1]
        h, w = int(cam.height * self.downsample), int(cam.width * self.downsample)
        self.img_wh = (w, h)
        if cam.model == 'SIMPLE_RADIAL':
            fx = fy = cam.params[0] * self.downsample
            cx, cy = cam.params[1] * self.downsample, cam.params[2] * self.downsample
        elif cam.model in ('PINHOLE', 'OPENCV'):
            fx, fy = cam.params[0] * self.downsample, cam.params[1] * self.downsample
            cx, cy = cam.params[2] * self.downsample, cam.params[3] * self.downsample
        else:
            raise ValueError(f"Please parse the intrinsics for camera model {cam.model}!")
        self.K = torch.FloatTensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
        self.directions = get_ray_directions(h, w, self.K)

    def read_meta(self, split, **kwargs):
        hdr = 'HDR-NeRF' in self.root_dir
        imdata = read_images_binary(os.path.join(self.root_dir, 'sparse/0/images.bin'))
        img_names = [imdata[k].name for k in imdata]
        perm = np.argsort(img_names)
        folder = f'images_{int(1 / self.downsample)}' if '360_v2' in self.root_dir and self.downsample < 1 \
            else 'images'
        img_paths = [os.path.join(self.root_dir, folder, name) for name in sorted(img_names)]
        bottom = np.array([[0, 0, 0, 1.]])
        w2c = np.stack([np.concatenate([np.concatenate([imdata[k].qvec2rotmat(), imdata[k].tvec.reshape(3, 1)], 1),
                                        bottom], 0) for k in imdata], 0)
        poses = np.linalg.inv(w2c)[perm, :3]  # (N_images, 3, 4) cam2world
        pts3d = read_points3d_binary(os.path.join(self.root_dir, 'sparse/0/points3D.bin'))
        pts3d = np.array([pts3d[k].xyz for k in pts3d])
        self.poses, self.pts3d, pose_avg = center_poses(poses, pts3d)
        scale = np.linalg.norm(self.poses[..., 3], axis=-1).min()
        self.poses[..., 3] /= scale
        self.pts3d /= scale
        self.blender_trans = np.eye(4)
        self.blender_trans[:3, :] = pose_avg
        self.blender_scale = scale
        self.rays = []
        if split == 'test_traj':
            self.poses = torch.FloatTensor(create_spheric_poses(1.2, self.poses[:, 1, 3].mean()))
            return
        if hdr:
            img_paths = self._hdr_nerf_split(split)
            self.rays = torch.stack([self._with_exposure_channel(p) for p in img_paths])
            self.poses = torch.FloatTensor(self.poses)
            return
        if split == 'train':
            keep = [i for i in range(len(img_paths)) if i % 8 != 0]
        elif split == 'test':
            keep = [i for i in range(len(img_paths)) if i % 8 == 0]
        else:
            keep = list(range(len(img_paths)))
        img_paths = [img_paths[i] for i in keep]
        self.poses = np.array([self.poses[i] for i in keep])
        self.rays = torch.stack([torch.FloatTensor(read_image(p, self.img_wh, blend_a=False)) for p in img_paths])
        self.poses = torch.FloatTensor(self.poses)

    def _hdr_nerf_split(self, split):
        """datasets/colmap.py:91-123: the split's image paths; sets unit_exposure_rgb and repeats
        self.poses once per exposure of the split."""
        if split not in ('train', 'test'):
            raise ValueError(f"split {split} is invalid for HDR-NeRF!")

        def pick(pattern):
            return sorted(glob.glob(os.path.join(self.root_dir, pattern)))

        if 'syndata' in self.root_dir:  # synthetic: the first 17 poses are test, the last 18 train
            self.unit_exposure_rgb = 0.73
            if split == 'train':
                self.poses = np.repeat(self.poses[-18:], 3, 0)
                return pick('train/*[024].png')
            self.poses = np.repeat(self.poses[:17], 2, 0)
            return pick('test/*[13].png')
        self.unit_exposure_rgb = 0.5  # real: even views train, odd views test
        if split == 'train':
            self.poses = np.tile(self.poses[::2], (3, 1, 1))
            return sum((pick(f'input_images/*{e}.jpg')[::2] for e in (0, 2, 4)), [])
        self.poses = np.tile(self.poses[1::2], (2, 1, 1))
        return sum((pick(f'input_images/*{e}.jpg')[1::2] for e in (1, 3)), [])

    def _with_exposure_channel(self, img_path):
        """(h*w, 4): the image's colours and its exposure (datasets/colmap.py:141-161)."""
        img = torch.FloatTensor(read_image(img_path, self.img_wh, blend_a=False))
        scene = os.path.basename(os.path.normpath(self.root_dir))
        if scene not in HDR_NERF_EXPOSURES:
            raise ValueError(f"no exposure table for HDR-NeRF scene {scene!r} (known: {sorted(HDR_NERF_EXPOSURES)})")
        e = int(os.path.splitext(os.path.basename(img_path))[0][-1])
        return torch.cat([img, HDR_NERF_EXPOSURES[scene][e] * torch.ones_like(img[:, :1])], 1)
