"""Encoder plugins looked up by ``core_method`` (reference ``heter_model_baseline.py:47-59``).

The LiDAR encoders: PointPillar (the hot path, reference ``opencood/models/heter_encoders.py:22-50``) and SECOND
(reference ``:52-81``; its sparse convolutions come from ``sub_modules/sparse_ops`` because spconv is not
available).  The camera encoder: LiftSplatShoot (reference ``:83-241``) over ``CamEncode_Resnet101``, the one camera encoder the PTQ surface
quantizes; its pooling runs on ``quantv2x_amd.lift_splat`` (the HIP stage on a GPU, the statements on the CPU) and never forms the
``[B, N, D, fH, fW, C]`` product.
"""
import numpy as np
import torch
import torch.nn as nn

from ..utils.camera_utils import gen_dx_bx
from .sub_modules.lss_submodule import CamEncode_Resnet101, features_and_depth

from .sub_modules.height_compression import HeightCompression
from .sub_modules.mean_vfe import MeanVFE
from .sub_modules.pillar_vfe import PillarVFE
from .sub_modules.point_pillar_scatter import PointPillarScatter
from .sub_modules.sparse_backbone_3d import VoxelBackBone8x


class PointPillar(nn.Module):
    def __init__(self, args):
        super().__init__()
        extent = np.array(args['lidar_range'][3:6]) - np.array(args['lidar_range'][0:3])
        # like the reference, the grid size is written back into the caller's config
        args['point_pillar_scatter']['grid_size'] = np.round(extent / np.array(args['voxel_size'])).astype(np.int64)
        self.pillar_vfe = PillarVFE(args['pillar_vfe'], num_point_features=4,
                                    voxel_size=args['voxel_size'], point_cloud_range=args['lidar_range'])
        self.scatter = PointPillarScatter(args['point_pillar_scatter'])

    def forward(self, data_dict, modality_name):
        src = data_dict[f'inputs_{modality_name}']
        batch = {k: src[k] for k in ('voxel_features', 'voxel_coords', 'voxel_num_points')}
        return self.scatter(self.pillar_vfe(batch))['spatial_features']


class SECOND(nn.Module):
    def __init__(self, args):
        super().__init__()
        rng = np.array(args['lidar_range'])
        grid_size = np.round((rng[3:6] - rng[:3]) / np.array(args['voxel_size'])).astype(np.int64)
        self.vfe = MeanVFE(args['mean_vfe'], args['mean_vfe']['num_point_features'])
        self.spconv_block = VoxelBackBone8x(args['spconv'], input_channels=args['spconv']['num_features_in'], grid_size=grid_size)
        self.map_to_bev = HeightCompression(args['map2bev'])

    def forward(self, data_dict, modality_name):
        src = data_dict[f'inputs_{modality_name}']
        batch = {k: src[k] for k in ('voxel_features', 'voxel_coords', 'voxel_num_points')}
        batch['batch_size'] = int(batch['voxel_coords'][:, 0].max()) + 1
        return self.map_to_bev(self.spconv_block(self.vfe(batch)))['spatial_features']


class LiftSplatShoot(nn.Module):
    """``args``: ``grid_conf`` (xbound, ybound, zbound, ddiscr, mode), ``data_aug_conf['final_dim']``, ``img_downsample``, ``img_features``,
    ``camera_encoder``, ``use_depth_gt``, ``depth_supervision`` -- the reference's yaml block (exemplar.yaml, modality m4).  ``dx``, ``bx``,
    ``nx`` and ``frustum`` follow the module's device (non-persistent buffers: the ``state_dict`` keys stay the reference's)."""

    def __init__(self, args):
        super().__init__()
        from ...lift_splat import create_frustum
        self.grid_conf, self.data_aug_conf = args['grid_conf'], args['data_aug_conf']
        dx, bx, nx = gen_dx_bx(self.grid_conf['xbound'], self.grid_conf['ybound'], self.grid_conf['zbound'])
        for name, t in (("dx", dx), ("bx", bx), ("nx", nx)):
            self.register_buffer(name, t.clone().detach(), persistent=False)
        self.depth_supervision = args['depth_supervision']
        self.downsample, self.camC = args['img_downsample'], args['img_features']
        self.register_buffer("frustum", self.create_frustum(), persistent=False)
        self.use_quickcumsum = True
        self.D = self.frustum.shape[0]
        self.camera_encoder_type = args['camera_encoder']
        if self.camera_encoder_type != 'Resnet101':
            raise NotImplementedError(f"camera_encoder {self.camera_encoder_type!r}: this plugin builds 'Resnet101', the encoder the PTQ surface "
                                      "quantizes (QuantLiftSplatShoot refuses EfficientNet)")
        self.camencode = CamEncode_Resnet101(self.D, self.camC, self.downsample, self.grid_conf['ddiscr'], self.grid_conf['mode'],
                                             args['use_depth_gt'], args['depth_supervision'])
        self._stages = {}

    def create_frustum(self):
        from ...lift_splat import create_frustum
        return create_frustum(self.data_aug_conf['final_dim'], self.downsample, self.grid_conf['ddiscr'], self.grid_conf['mode'])

    def get_cam_feats(self, x):
        """images [B, N, 3 | 4, H, W] -> (depth items, depth [B*N, D, fH, fW], 'logits' | 'probs', features [B*N, C, fH, fW]): the two
        factors of the reference's product, not the product"""
        b, n, c, h, w = x.shape
        items, depth, mode, feats = features_and_depth(self.camencode, x.view(b * n, c, h, w))
        want = (h // self.downsample, w // self.downsample)
        if tuple(feats.shape[-2:]) != want:
            raise ValueError(f"images of {h} x {w} leave the encoder as {tuple(feats.shape[-2:])}, not (H // downsample, W // downsample) = {want}")
        return items, depth, mode, feats

    def get_voxels(self, x, rots, trans, intrins, post_rots, post_trans):
        items, depth, mode, feats = self.get_cam_feats(x)
        return pool_bev(self, x.shape[0], x.shape[1], depth, mode, feats, rots, trans, intrins, post_rots, post_trans), items

    def forward(self, data_dict, modality_name):
        src = data_dict[f'inputs_{modality_name}']
        x, items = self.get_voxels(*(src[k] for k in ('imgs', 'rots', 'trans', 'intrins', 'post_rots', 'post_trans')))
        if self.depth_supervision:
            self.depth_items = items
        return x


def pool_bev(lss, b, n, depth, mode, feats, rots, trans, intrins, post_rots, post_trans):
    """The voxel pooling of ``LiftSplatShoot`` and of its quantized wrapper -> BEV [B, C * Z, Y, X].  On a GPU the HIP stage
    (``GpuLiftSplat``, one per (B, N), re-planned on every call: the matrices are arguments here); on the CPU the cells of
    ``lift_splat.cells_statement`` and one ``index_add_`` per depth bin."""
    from ... import lift_splat as ls
    depth, feats = depth.detach().float().contiguous(), feats.detach().float().contiguous()
    if feats.is_cuda:
        stage = lss._stages.get((b, n))
        if stage is None:
            stage = lss._stages[(b, n)] = ls.GpuLiftSplat(lss.grid_conf, lss.data_aug_conf['final_dim'], lss.downsample, lss.camC, n, b, feats.device)
        return stage.plan(rots, trans, intrins, post_rots, post_trans)(depth, feats, mode).clone()
    cells = ls.cells_statement(ls.geometry_statement(lss.frustum, rots, trans, intrins, post_rots, post_trans), lss.dx, lss.bx, lss.nx)
    cells = torch.from_numpy(cells.astype(np.int64))                                    # [B, N, D, fH, fW]
    nx, ny, nz = (int(v) for v in lss.nx)
    c, d = feats.shape[1], depth.shape[1]
    prob = (torch.softmax(depth, dim=1) if mode == "logits" else depth).view(b, n, d, -1)
    rows = feats.view(b, n, c, -1).permute(0, 1, 3, 2)                                  # [B, N, fH*fW, C]
    out = torch.zeros((b, nz * ny * nx + 1, c), dtype=feats.dtype)                      # the last row collects the dropped points
    for s in range(b):
        for k in range(d):
            idx = cells[s, :, k].reshape(-1)
            idx = torch.where(idx < 0, torch.full_like(idx, nz * ny * nx), idx)
            out[s].index_add_(0, idx, (prob[s, :, k].unsqueeze(-1) * rows[s]).reshape(-1, c))
    return out[:, :-1].view(b, nz, ny, nx, c).permute(0, 1, 4, 2, 3).reshape(b, nz * c, ny, nx)
