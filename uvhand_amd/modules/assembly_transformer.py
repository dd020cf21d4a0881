"""``DeformableTransformer`` / ``DeformableTransformerDecoder`` of UVHand's AssemblyHands model
(models/assembly_transformer.py:23-251 and :387-465, built by models/assembly_detr.py), drop-in.  Exported from
``uvhand_amd.modules`` as ``AssemblyDeformableTransformer`` / ``AssemblyDeformableTransformerDecoder``.

The encoder and decoder layers are the ARCTIC file's (no hunk between the two files' layer classes), so they are this
package's (modules/deformable_layers.py); what differs is this transformer class and the decoder stack.

Contract kept: the constructor signatures and defaults (``cfg=None`` stored as ``self.cfg``; no ``two_stage_learn_xy``);
sub-modules with the same names in the same creation order (``encoder, decoder, level_embed``, then ``enc_output,
enc_output_norm, pos_trans`` — one ``nn.Linear(2d, 2d)`` — ``pos_trans_norm``, or ``reference_points``); the same
``_reset_parameters``, so a construction under one ``torch.manual_seed`` gives the reference's ``state_dict`` bit for bit;
``get_valid_ratio`` / ``get_proposal_pos_embed`` / ``gen_encoder_output_proposals`` / ``forward`` with the reference's
signatures and return values (``forward``: the six-tuple, ``None`` x 3 when not two-stage).  The decoder's per-layer heads
``cls_embed`` / ``keypoint_embed`` / ``obj_keypoint_embed`` are attached from outside, as models/assembly_detr.py:100-118
does.

What is MI355X-specific: the stacks and the flatten are this package's; the decoder's refinement after every layer is one
HIP launch without a host synchronisation (the reference's boolean-mask add is a ``nonzero``), so a decoder forward can be
captured in a graph; the two-stage block's proposals (last level only, as :184) and selection are HIP kernels too
(functions/assembly_func.py).  The heads stay ordinary modules (hooks and checkpoints see them); inside
the decoder they run under ``no_grad``, since their outputs there only feed the detached refinement — unreachable by
autograd in the reference as well.
"""
import torch
from torch import nn
from torch.nn.init import constant_, normal_, xavier_uniform_

from ..functions import assembly_func as AF
from ..functions import two_stage_func as TS
from ..functions.layernorm_func import add_layer_norm
from ..functions.linear_func import bracket_linear
from ..utils.transformer_inputs import decoder_reference_points, flatten_feature_levels
from ..utils.transformer_inputs import get_valid_ratio as _valid_ratio
from .deformable_layers import (DeformableTransformerDecoderLayer, DeformableTransformerEncoder, DeformableTransformerEncoderLayer,
                                _get_clones)
from .deformable_transformer import _level_hw
from .ms_deform_attn import MSDeformAttn


class DeformableTransformerDecoder(nn.Module):
    """``num_layers`` copies of a decoder layer (models/assembly_transformer.py:387-465).  With ``cls_embed`` and
    ``keypoint_embed`` attached (``with_box_refine``) the reference points are refined after every layer: 2-d or 42-d in,
    42-d out, moved by the keypoint head on the queries whose class argmax is not 0 (functions/assembly_func.refine)."""

    def __init__(self, decoder_layer, num_layers, return_intermediate=False, cfg=None):
        super().__init__()
        self.layers = _get_clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.return_intermediate = return_intermediate
        self.keypoint_embed = None
        self.obj_keypoint_embed = None
        self.cls_embed = None
        self.cfg = cfg

    def _refine(self, lid, output, reference_points):
        if self.cls_embed is None:       # the reference reads hand_idx, which only the class head defines (:412-442)
            raise UnboundLocalError("keypoint refinement needs decoder.cls_embed (the reference's hand_idx is unbound)")
        with torch.no_grad():
            cls_out = self.cls_embed[lid](output)
            tmp = self.keypoint_embed[lid](output)
        return AF.refine(reference_points, cls_out, tmp)

    def forward(self, tgt, reference_points, src, src_spatial_shapes, src_level_start_index, src_valid_ratios,
                query_pos=None, src_padding_mask=None):
        output = tgt
        intermediate, intermediate_reference_points = [], []
        for lid, layer in enumerate(self.layers):
            if reference_points.shape[-1] not in (2, 42):
                raise AssertionError("reference_points must have 2 or 42 coordinates per query")
            reference_points_input = decoder_reference_points(reference_points, src_valid_ratios)
            output = layer(output, query_pos, reference_points_input, src, src_spatial_shapes, src_level_start_index,
                           src_padding_mask)
            # the class head alone (keypoint_embed None) only feeds a dead argmax in the reference (:412-420): skipped
            if self.keypoint_embed is not None:
                reference_points = self._refine(lid, output, reference_points)
            if self.return_intermediate:
                intermediate.append(output)
                intermediate_reference_points.append(reference_points)
        if self.return_intermediate:
            return torch.stack(intermediate), torch.stack(intermediate_reference_points)
        return output, reference_points


class DeformableTransformer(nn.Module):
    def __init__(self, d_model=256, nhead=8, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=1024, dropout=0.1,
                 activation="relu", return_intermediate_dec=False, num_feature_levels=4, dec_n_points=4, enc_n_points=4,
                 two_stage=False, two_stage_num_proposals=300, cfg=None):
        super().__init__()
        self.d_model = d_model
        self.nhead = nhead
        self.two_stage = two_stage
        self.two_stage_num_proposals = two_stage_num_proposals
        self.n_levels = num_feature_levels
        self.n_points = dec_n_points
        self.cfg = cfg

        encoder_layer = DeformableTransformerEncoderLayer(d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead,
                                                          enc_n_points)
        self.encoder = DeformableTransformerEncoder(encoder_layer, num_encoder_layers)
        decoder_layer = DeformableTransformerDecoderLayer(d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead,
                                                          dec_n_points)
        self.decoder = DeformableTransformerDecoder(decoder_layer, num_decoder_layers, return_intermediate_dec, cfg)

        self.level_embed = nn.Parameter(torch.Tensor(num_feature_levels, d_model))

        if two_stage:
            self.enc_output = nn.Linear(d_model, d_model)
            self.enc_output_norm = nn.LayerNorm(d_model)
            self.pos_trans = nn.Linear(d_model * 2, d_model * 2)
            self.pos_trans_norm = nn.LayerNorm(d_model * 2)
        else:
            self.reference_points = nn.Linear(d_model, 2)

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

    def get_proposal_pos_embed(self, proposals):
        """[N, L, c] -> [N, L, 128 c]: per coordinate 64 (sin, cos) pairs of sigmoid(x) * 2pi / 10000^(2i/128) (:74-87; the
        forward does not call it)."""
        return TS.pos_embed_composition(proposals)

    def gen_encoder_output_proposals(self, memory, memory_padding_mask, spatial_shapes):
        """(enc_output_norm(enc_output(memory with padded / out-of-range rows zeroed)), output_proposals [N, S, 2])."""
        output_memory, output_proposals = AF.encoder_output_proposals(memory, memory_padding_mask, _level_hw(spatial_shapes))
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
            # the last level only (:184); its start as a host int, so the slice costs no device read-back
            last = sum(h * w for h, w in level_hw[:-1])
            output_memory, output_proposals = self.gen_encoder_output_proposals(memory[:, last:], mask_flatten[:, last:],
                                                                                level_hw[-1:])
            nl = self.decoder.num_layers
            enc_outputs_class = self.decoder.cls_embed[nl](output_memory)
            enc_outputs_hand_coord_unact = self.decoder.keypoint_embed[nl](output_memory)
            enc_outputs_obj_coord_unact = self.decoder.obj_keypoint_embed[nl](output_memory)
            # the proposal's (x, y) under every keypoint's (x, y, z): ordinary differentiable in-place adds, as in the reference
            enc_outputs_hand_coord_unact[..., 0::3] += output_proposals[..., 0:1]
            enc_outputs_hand_coord_unact[..., 1::3] += output_proposals[..., 1:2]
            enc_outputs_obj_coord_unact[..., 0::3] += output_proposals[..., 0:1]
            enc_outputs_obj_coord_unact[..., 1::3] += output_proposals[..., 1:2]

            reference_points = AF.select_queries(enc_outputs_class, enc_outputs_hand_coord_unact, enc_outputs_obj_coord_unact)
            init_reference_out = reference_points
        else:
            reference_points = None
        # both modes take the queries from query_embed (the reference's two-stage pos_trans route is commented out, :228-230)
        query_embed, tgt = torch.split(query_embed, c, dim=1)
        query_embed = query_embed.unsqueeze(0).expand(bs, -1, -1)
        tgt = tgt.unsqueeze(0).expand(bs, -1, -1)
        if not self.two_stage:
            reference_points = self.reference_points(query_embed).sigmoid()
            init_reference_out = reference_points

        hs, inter_references = self.decoder(tgt, reference_points, memory, spatial_shapes, level_start_index, valid_ratios,
                                            query_embed, mask_flatten)
        if self.two_stage:
            return (hs, init_reference_out, inter_references, enc_outputs_class, enc_outputs_hand_coord_unact,
                    enc_outputs_obj_coord_unact)
        return hs, init_reference_out, inter_references, None, None, None
