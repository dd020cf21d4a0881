"""Drop-in SmoothNet modules (models/smoothnet.py:7-178 and 202-217): ``SmootherResBlock``, ``Smoother``, ``MotionSmoother``,
``ArcticSmoother`` and ``SmoothCriterion``.

Constructors, submodule names and creation order and ``ArcticSmoother._reset_parameters`` are the reference's, so a
reference checkpoint loads with ``strict=True`` and one seed builds a bit-identical ``state_dict``.  ``MotionSmoother.forward``
and ``ArcticSmoother.forward`` run through one autograd node (``functions.smoother_func.motion_smoothers``): on CUDA fp32 the
nine MotionSmoother calls of ``ArcticSmoother`` take 9 HIP launches forward instead of several hundred.  Dropout then draws
from the kernels' own hash, not from ``nn.Dropout``'s stream.  ``SmootherResBlock`` and ``Smoother`` keep the reference's
forward (they are the parameter containers; called on their own they run torch).

``SmoothCriterion`` keeps the reference's constructor, ``weight_dict`` and ``forward(args, data, targets, meta_info)`` over
``prepare_data``'s ``XDict``; its losses come from ``uvhand_amd.smooth_loss.compute_smoothnet_loss`` (three HIP launches
forward, one backward, no host sync).  ``acc_grad=True`` lets ``acc/h`` and ``acc/o`` carry gradients, which the reference's
numpy round trip drops."""
import torch
from torch import nn

from ..functions.smoother_func import motion_smoothers

__all__ = ["SmootherResBlock", "Smoother", "MotionSmoother", "ArcticSmoother", "SmoothCriterion"]


class SmootherResBlock(nn.Module):
    def __init__(self, in_channels, hidden_channels, dropout=0.9):
        super().__init__()
        self.linear1 = nn.Linear(in_channels, hidden_channels)
        self.linear2 = nn.Linear(hidden_channels, in_channels)
        self.lrelu = nn.LeakyReLU(0.2, inplace=True)
        self.dropout = nn.Dropout(p=dropout, inplace=True)

    def forward(self, x):
        identity = x
        x = self.linear1(x)
        x = self.dropout(x)
        x = self.lrelu(x)
        x = self.linear2(x)
        x = self.dropout(x)
        x = self.lrelu(x)
        return x + identity


class Smoother(nn.Module):
    def __init__(self, window_size, output_size, hidden_size=512, res_hidden_size=256, num_blocks=3, dropout=0.9):
        super().__init__()
        self.window_size = window_size
        self.output_size = output_size
        self.hidden_size = hidden_size
        self.res_hidden_size = res_hidden_size
        self.num_blocks = num_blocks
        self.dropout = dropout

        self.encoder = nn.Sequential(
            nn.Linear(window_size, hidden_size),
            nn.LeakyReLU(0.1, inplace=True)
        )
        self.res_blocks = nn.Sequential(*[
            SmootherResBlock(in_channels=hidden_size, hidden_channels=res_hidden_size, dropout=dropout)
            for _ in range(num_blocks)])
        self.decoder = nn.Linear(hidden_size, output_size)

    def forward(self, x):
        x = self.encoder(x)
        x = self.res_blocks(x)
        return self.decoder(x)


class MotionSmoother(nn.Module):
    def __init__(self, window_size, output_size, hidden_size=512, res_hidden_size=256, num_blocks=3, dropout=0.9):
        super().__init__()
        self.window_size = window_size
        self.output_size = output_size
        self.hidden_size = hidden_size
        self.res_hidden_size = res_hidden_size
        self.num_blocks = num_blocks
        self.dropout = dropout

        self.pos_smoother = Smoother(window_size, output_size, hidden_size, res_hidden_size, num_blocks, dropout)
        self.vel_smoother = Smoother(window_size - 1, output_size, hidden_size, res_hidden_size, num_blocks, dropout)
        self.acc_smoother = Smoother(window_size - 2, output_size, hidden_size, res_hidden_size, num_blocks, dropout)
        self.fusion_layer = nn.Linear(3 * output_size, output_size)

    def forward(self, x):
        """x [N, T, C] -> [N, output_size, C] (the reference returns the same values as a permuted view)."""
        return motion_smoothers([(0, x)], [self], self.training)[0]


# ArcticSmoother's nine calls: (module attribute, output width) in the reference's return order
_ARCTIC_CALLS = (("mano_root_smoother", 3), ("mano_root_smoother", 3), ("obj_root_smoother", 3),
                 ("mano_pose_smoother", 48), ("mano_pose_smoother", 48),
                 ("mano_shape_smoother", 10), ("mano_shape_smoother", 10),
                 ("obj_rot_smoother", 3), ("obj_rad_smoother", 1))


class ArcticSmoother(nn.Module):
    def __init__(self, batch_size, window_size):
        super().__init__()

        self.mano_pose_smoother = MotionSmoother(window_size, window_size)
        self.mano_shape_smoother = MotionSmoother(window_size, window_size)
        self.obj_rot_smoother = MotionSmoother(window_size, window_size)
        self.obj_rad_smoother = MotionSmoother(window_size, window_size)
        self.mano_root_smoother = MotionSmoother(window_size, window_size)
        self.obj_root_smoother = MotionSmoother(window_size, window_size)

        self.batch_size = batch_size
        self.window_size = window_size

        self._reset_parameters()

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, output):
        """output: ([root_l, root_r, root_o], [mano_pose_l, mano_pose_r], [mano_shape_l, mano_shape_r], [obj_rot, obj_rad]),
        each [B * T, C] (get_arctic_item's result); returns the smoothed parameters in the same structure."""
        B = self.batch_size
        T = self.window_size
        root, mano_pose, mano_shape, obj_angle = output
        root_l, root_r, root_o = root
        mano_pose_l, mano_pose_r = mano_pose
        mano_shape_l, mano_shape_r = mano_shape
        obj_rot, obj_rad = obj_angle
        inputs = (root_l, root_r, root_o, mano_pose_l, mano_pose_r, mano_shape_l, mano_shape_r, obj_rot, obj_rad)
        names = []
        for name, _ in _ARCTIC_CALLS:
            if name not in names:
                names.append(name)
        modules = [getattr(self, n) for n in names]
        calls = [(names.index(name), x.view(B, T, -1)) for (name, _), x in zip(_ARCTIC_CALLS, inputs)]
        outs = motion_smoothers(calls, modules, self.training)
        r = [o.reshape(-1, w) for o, (_, w) in zip(outs, _ARCTIC_CALLS)]
        return r[0:3], r[3:5], r[5:7], r[7:9]


class SmoothCriterion(nn.Module):
    """The SmoothNet criterion: ``forward(args, data, targets, meta_info)`` over ``prepare_data``'s ``XDict`` returns
    ``{"loss/cd", "acc/h", "acc/o"}``; ``weight_dict`` is the caller's to apply.  It has no parameters."""

    def __init__(self, batch_size, window_size, weight_dict, pre_process_models, acc_grad=False):
        super().__init__()
        self.batch_size, self.window_size = batch_size, window_size
        self.weight_dict, self.pre_process_models = weight_dict, pre_process_models
        self.acc_grad = acc_grad

    def forward(self, args, data, targets, meta_info):
        from ..smooth_loss import compute_smoothnet_loss       # resolved on first use: importing the modules stays light
        return dict(compute_smoothnet_loss(data.search("pred.", ""), data.search("targets.", ""), meta_info,
                                           self.pre_process_models, args.img_res, acc_grad=self.acc_grad))
