"""``DeformableTransformer`` — the class UVHand's model builds (``build_deforamble_transformer``,
models/arctic_transformer.py:474-488, returns ``DeformableTransformer``, :23-259), drop-in.

Contract kept: the constructor's signature and defaults (``two_stage_learn_xy`` included); sub-modules with the same names in
the same creation order (``encoder, decoder, level_embed``, then ``enc_output, enc_output_norm, pos_trans`` — the same
``nn.Sequential`` of Linear / ReLU x 3, so the keys stay ``pos_trans.0.weight`` … — ``pos_trans_norm`` or
``reference_points``, then ``two_stage_learn_xy``); the same ``_reset_parameters``, so a construction under one
``torch.manual_seed`` consumes the random stream as the reference's does and gives a bit-identical ``state_dict``;
``get_valid_ratio`` / ``get_proposal_pos_embed`` / ``gen_encoder_output_proposals`` / ``forward`` with the reference's
signatures and return values (``forward``: the six-tuple, ``None`` x 3 when not two-stage).  The per-layer heads
(``decoder.cls_embed`` / ``key_embed`` / ``obj_key_embed``, one more than there are decoder layers in two-stage mode) are
attached from outside, as the reference's model does (models/actic_detr.py:130-149).

What is MI355X-specific: the stacks are this package's (MSDeformAttn, fused add + LayerNorm and FFN, the attention core);
the flatten is one kernel per direction (utils/transformer_inputs.py); the two-stage block is functions/two_stage_func.py —
the proposals in one pass, the query selection in one launch without a host synchronisation, and ``pos_trans[0]`` fused with
the proposal embedding so that the [N, Q, 5376] sin / cos table is never written.
"""
import math

import torch
from torch import nn
from torch.nn.init import constant_, normal_, xavier_uniform_

from ..functions import two_stage_func as TS
from ..functions.layernorm_func import add_layer_norm
from ..functions.linear_func import bracket_linear
from ..utils.transformer_inputs import flatten_feature_levels
from ..utils.transformer_inputs import get_valid_ratio as _valid_ratio
from .deformable_layers import (DeformableTransformerDecoder, DeformableTransformerDecoderLayer, DeformableTransformerEncoder,
                                DeformableTransformerEncoderLayer)
from .ms_deform_attn import MSDeformAttn


def _level_hw(spatial_shapes):
    """[(H, W)] as Python ints from a list of pairs or an [L, 2] tensor (a tensor is read back once)."""
    if torch.is_tensor(spatial_shapes):
        spatial_shapes = spatial_shapes.tolist()
    return [(int(h), int(w)) for h, w in spatial_shapes]


class DeformableTransformer(nn.Module):
    def __init__(self, d_model=256, nhead=8, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=1024, dropout=0.1,
                 activation="relu", return_intermediate_dec=False, num_feature_levels=4, dec_n_points=4, enc_n_points=4,
                 two_stage=False, two_stage_num_proposals=300, two_stage_learn_xy=True):
        super().__init__()
        self.d_model = d_model
        self.nhead = nhead
        self.two_stage = two_stage
        self.two_stage_num_proposals = two_stage_num_proposals
        self.n_levels = num_feature_levels
        self.n_points = dec_n_points
        self.two_stage_learn_xy = None

        encoder_layer = DeformableTransformerEncoderLayer(d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead,
                                                          enc_n_points)
        self.encoder = DeformableTransformerEncoder(encoder_layer, num_encoder_layers)
        decoder_layer = DeformableTransformerDecoderLayer(d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead,
                                                          dec_n_points)
        self.decoder = DeformableTransformerDecoder(decoder_layer, num_decoder_layers, return_intermediate_dec)

        self.level_embed = nn.Parameter(torch.Tensor(num_feature_levels, d_model))

        if two_stage:
            self.enc_output = nn.Linear(d_model, d_model)
            self.enc_output_norm = nn.LayerNorm(d_model)
            # the 42 x 128 sin / cos features of the selected refpoints -> 2 * d_model (query_pos, tgt)
            self.pos_trans = nn.Sequential(nn.Linear(5376, 1024), nn.ReLU(), nn.Linear(1024, 1024), nn.ReLU(),
                                           nn.Linear(1024, 512), nn.ReLU())
            self.pos_trans_norm = nn.LayerNorm(d_model * 2)
        else:
            self.reference_points = nn.Linear(d_model, 2)

        # the proposal predicts the root (x, y); the other 20 keypoints' (x, y) start from a learned offset
        if two_stage and two_stage_learn_xy:
            self.two_stage_learn_xy = nn.Embedding(1, 40)

        self._reset_parameters()

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, MSDeformAttn):
                m._reset_parameters()
        if not self.two_stage:
            xavier_uniform_(self.reference_points.weight.data, gain=1.0)
            constant_(self.reference_points.bias.data, 0.)
        normal_(self.level_embed)
        if self.two_stage_learn_xy is not None:
            nn.init.constant_(self.two_stage_learn_xy.weight, math.log(0.05 / (1 - 0.05)))

    def get_proposal_pos_embed(self, proposals):
        """[N, L, 42] -> [N, L, 5376]: per coordinate 64 (sin, cos) pairs of sigmoid(x) * 2pi / 10000^(2i/128)."""
        return TS.proposal_pos_embed(proposals)

    def gen_encoder_output_proposals(self, memory, memory_padding_mask, spatial_shapes, learnedxy):
        """(enc_output_norm(enc_output(memory with padded / out-of-range rows zeroed)), output_proposals [N, S, 42])."""
        output_memory, output_proposals = TS.encoder_output_proposals(memory, memory_padding_mask, _level_hw(spatial_shapes),
                                                                      learnedxy)
        output_memory = add_layer_norm(bracket_linear(output_memory, self.enc_output), None, self.enc_output_norm)
        return output_memory, output_proposals

    def get_valid_ratio(self, mask):
        return _valid_ratio(mask)

    def forward(self, srcs, masks, pos_embeds, query_embed=None):
        assert self.two_stage or query_embed is not None
        level_hw = [(int(s.shape[2]), int(s.shape[3])) for s in srcs]
        (src_flatten, mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index,
         valid_ratios) = flatten_feature_levels(srcs, masks, pos_embeds, self.level_embed)

        memory = self.encoder(src_flatten, spatial_shapes, level_start_index, valid_ratios, lvl_pos_embed_flatten, mask_flatten)

        bs, _, c = memory.shape
        if self.two_stage:
            learnedxy = self.two_stage_learn_xy.weight[0] if self.two_stage_learn_xy is not None else None
            output_memory, output_proposals = self.gen_encoder_output_proposals(memory, mask_flatten, level_hw, learnedxy)
            nl = self.decoder.num_layers
            enc_outputs_class = self.decoder.cls_embed[nl](output_memory)
            enc_outputs_hand_coord_unact = self.decoder.key_embed[nl](output_memory)
            enc_outputs_obj_coord_unact = self.decoder.obj_key_embed[nl](output_memory)
            # the root's (x, y) proposal under every keypoint: ordinary differentiable in-place adds, as in the reference
            enc_outputs_hand_coord_unact[..., 0::2] += output_proposals[..., 0:1]
            enc_outputs_hand_coord_unact[..., 1::2] += output_proposals[..., 1:2]
            enc_outputs_obj_coord_unact[..., 0::2] += output_proposals[..., 0:1]
            enc_outputs_obj_coord_unact[..., 1::2] += output_proposals[..., 1:2]

            refpoint_embed_undetach, reference_points = TS.select_queries(
                enc_outputs_class, enc_outputs_hand_coord_unact, enc_outputs_obj_coord_unact, output_proposals,
                self.two_stage_num_proposals)
            init_reference_out = reference_points
            pos_trans_out = TS.pos_trans_embed(self.pos_trans, self.pos_trans_norm, refpoint_embed_undetach)
            query_embed, tgt = torch.split(pos_trans_out, c, dim=2)
        else:
            query_embed, tgt = torch.split(query_embed, c, dim=1)
            query_embed = query_embed.unsqueeze(0).expand(bs, -1, -1)
            tgt = tgt.unsqueeze(0).expand(bs, -1, -1)
            reference_points = self.reference_points(query_embed).sigmoid()
            init_reference_out = reference_points

        hs, inter_references = self.decoder(tgt, reference_points, memory, spatial_shapes, level_start_index, valid_ratios,
                                            query_embed, mask_flatten)
        if self.two_stage:
            return (hs, init_reference_out, inter_references, enc_outputs_class, enc_outputs_hand_coord_unact,
                    enc_outputs_obj_coord_unact)
        return hs, init_reference_out, inter_references, None, None, None
