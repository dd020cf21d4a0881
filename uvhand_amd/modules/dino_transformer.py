"""``TransformerDecoder`` / ``DeformableTransformerDecoderLayer`` of UVHand's DINO model
(models/dino/deformable_transformer.py:627-827 and :886-1058, built by models/dino/dino.py), drop-in.  Exported from
``uvhand_amd.modules`` as ``DinoTransformerDecoder`` / ``DinoDeformableTransformerDecoderLayer``.

This is not the ARCTIC decoder of modules/deformable_layers.py: the tensors are sequence-first ([L, N, C]); there is no fixed
``query_pos`` — every layer recomputes it from the current reference points through ``ref_point_head``; the refinement's
result is handed to the model undetached ("look forward twice", dino.py:329-337); and the final ``norm`` is applied to every
intermediate output.

Contract kept: the constructor arguments and defaults, the sub-module names (``cross_attn, dropout1, norm1, self_attn,
dropout2, norm2, linear1, dropout3, linear2, dropout4, norm3`` / ``layers, norm, ref_point_head``), hence the checkpoint
keys; ``forward`` / ``forward_sa`` / ``forward_ca`` / ``forward_ffn`` / ``rm_self_attn_modules`` with the reference's
signatures; the decoder's return value (the lists of [N, L, C] normed outputs and of ``num_layers + 1`` reference points).
``class_embed`` / ``key_embed`` / ``obj_key_embed`` / ``bbox_embed`` and ``rm_detach`` start as ``None`` and are attached from
outside, as dino.py:200-202 does.  What every ``config/DINO/*.py`` sets is required: ``decoder_sa_type='sa'``,
``use_deformable_box_attn=False``, ``deformable_decoder=True``, ``rm_dec_query_scale=True``; anything else raises
``NotImplementedError`` at construction.

What is MI355X-specific: a decoder step runs on this package's pieces — ``self_attention`` (with DINO's denoising mask the
masked, long-sequence core), ``MSDeformAttn``, ``fused_ffn``, ``add_layer_norm``, and functions/dino_func.py's ``query_pos``
and ``refine`` — and makes no host synchronisation, so forward plus backward can be captured in a graph.
``decoder_query_perturber``, ``dec_layer_dropout_prob``, ``use_detached_boxes_dec_out``, ``rm_detach`` and
``dec_layer_number`` keep the reference's Python form (``rm_detach=['dec']`` makes the reference points require grad, which
selects the compositions)."""
import copy
import random

import torch.nn.functional as F
from torch import nn

from ..functions import dino_func as DF
from ..functions.attention_func import self_attention
from ..functions.layernorm_func import add_layer_norm
from ..functions.linear_func import fused_ffn
from ..utils.transformer_inputs import decoder_reference_points
from .detr import MLP
from .ms_deform_attn import MSDeformAttn


def _get_activation_fn(activation):
    """models/dino/utils.py:122-135: the same five names, the same exception type."""
    if activation == "relu":
        return F.relu
    if activation == "gelu":
        return F.gelu
    if activation == "glu":
        return F.glu
    if activation == "prelu":
        return nn.PReLU()
    if activation == "selu":
        return F.selu
    raise RuntimeError("activation should be relu/gelu, not %s." % activation)


def _get_clones(module, n, layer_share=False):
    if layer_share:
        return nn.ModuleList([module for _ in range(n)])
    return nn.ModuleList([copy.deepcopy(module) for _ in range(n)])


class DeformableTransformerDecoderLayer(nn.Module):
    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4,
                 use_deformable_box_attn=False, box_attn_type='roi_align', key_aware_type=None, decoder_sa_type='ca',
                 module_seq=['sa', 'ca', 'ffn']):
        super().__init__()
        self.module_seq = module_seq
        assert sorted(module_seq) == ['ca', 'ffn', 'sa']
        assert decoder_sa_type in ['sa', 'ca_label', 'ca_content']
        if use_deformable_box_attn:
            raise NotImplementedError("use_deformable_box_attn=True (MSDeformableBoxAttention) is not part of this package")
        if decoder_sa_type != 'sa':
            raise NotImplementedError("decoder_sa_type=%r: every config/DINO file sets 'sa', the only form built here"
                                      % decoder_sa_type)
        self.cross_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation)
        self.dropout3 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout4 = nn.Dropout(dropout)
        self.norm3 = nn.LayerNorm(d_model)
        self.key_aware_type = key_aware_type
        self.key_aware_proj = None
        self.decoder_sa_type = decoder_sa_type

    def rm_self_attn_modules(self):
        self.self_attn = None
        self.dropout2 = None
        self.norm2 = None

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, tgt):
        tgt2 = fused_ffn(tgt, self.linear1, self.activation, self.dropout3, self.linear2)
        return add_layer_norm(tgt, self.dropout4(tgt2), self.norm3)

    def forward_sa(self, tgt, tgt_query_pos=None, tgt_query_sine_embed=None, tgt_key_padding_mask=None,
                   tgt_reference_points=None, memory=None, memory_key_padding_mask=None, memory_level_start_index=None,
                   memory_spatial_shapes=None, memory_pos=None, self_attn_mask=None, cross_attn_mask=None):
        if self.self_attn is not None:
            q = self.with_pos_embed(tgt, tgt_query_pos)
            # sequence-first, as the reference feeds nn.MultiheadAttention; with the denoising mask the masked, long core
            tgt2 = self_attention(self.self_attn, q, tgt, self_attn_mask)
            tgt = add_layer_norm(tgt, self.dropout2(tgt2), self.norm2)
        return tgt

    def forward_ca(self, tgt, tgt_query_pos=None, tgt_query_sine_embed=None, tgt_key_padding_mask=None,
                   tgt_reference_points=None, memory=None, memory_key_padding_mask=None, memory_level_start_index=None,
                   memory_spatial_shapes=None, memory_pos=None, self_attn_mask=None, cross_attn_mask=None):
        if self.key_aware_type is not None:
            if self.key_aware_type == 'mean':
                tgt = tgt + memory.mean(0, keepdim=True)
            else:
                raise NotImplementedError("Unknown key_aware_type: {}".format(self.key_aware_type))
        tgt2 = self.cross_attn(self.with_pos_embed(tgt, tgt_query_pos).transpose(0, 1),
                               tgt_reference_points.transpose(0, 1).contiguous(), memory.transpose(0, 1), memory_spatial_shapes,
                               memory_level_start_index, memory_key_padding_mask).transpose(0, 1)
        return add_layer_norm(tgt, self.dropout1(tgt2), self.norm1)

    def forward(self, tgt, tgt_query_pos=None, tgt_query_sine_embed=None, tgt_key_padding_mask=None, tgt_reference_points=None,
                memory=None, memory_key_padding_mask=None, memory_level_start_index=None, memory_spatial_shapes=None,
                memory_pos=None, self_attn_mask=None, cross_attn_mask=None):
        args = (tgt_query_pos, tgt_query_sine_embed, tgt_key_padding_mask, tgt_reference_points, memory, memory_key_padding_mask,
                memory_level_start_index, memory_spatial_shapes, memory_pos, self_attn_mask, cross_attn_mask)
        for funcname in self.module_seq:
            if funcname == 'ffn':
                tgt = self.forward_ffn(tgt)
            elif funcname == 'ca':
                tgt = self.forward_ca(tgt, *args)
            elif funcname == 'sa':
                tgt = self.forward_sa(tgt, *args)
            else:
                raise ValueError('unknown funcname {}'.format(funcname))
        return tgt


class TransformerDecoder(nn.Module):
    hand_classes = (12, 13)                       # left / right hand in the ARCTIC label set (:787)

    def __init__(self, decoder_layer, num_layers, norm=None, return_intermediate=False, d_model=256, query_dim=4,
                 modulate_hw_attn=False, num_feature_levels=1, deformable_decoder=False, decoder_query_perturber=None,
                 dec_layer_number=None, rm_dec_query_scale=False, dec_layer_share=False, dec_layer_dropout_prob=None,
                 use_detached_boxes_dec_out=False):
        super().__init__()
        if num_layers > 0:
            self.layers = _get_clones(decoder_layer, num_layers, layer_share=dec_layer_share)
        else:
            self.layers = []
        self.num_layers = num_layers
        self.norm = norm
        self.return_intermediate = return_intermediate
        assert return_intermediate, "support return_intermediate only"
        self.query_dim = query_dim
        assert query_dim in [2, 4], "query_dim should be 2/4 but {}".format(query_dim)
        self.num_feature_levels = num_feature_levels
        self.use_detached_boxes_dec_out = use_detached_boxes_dec_out
        if not deformable_decoder:
            raise NotImplementedError("deformable_decoder=False (the query_pos_sine_scale / ref_anchor_head form) is not built here")
        if not rm_dec_query_scale:
            raise NotImplementedError                # as the reference does (:667)

        self.ref_point_head = MLP(d_model, d_model, d_model, 2)
        self.query_pos_sine_scale = None
        self.query_scale = None
        self.bbox_embed = None
        self.class_embed = None
        self.key_embed = None
        self.obj_key_embed = None

        self.d_model = d_model
        self.modulate_hw_attn = modulate_hw_attn
        self.deformable_decoder = deformable_decoder
        self.ref_anchor_head = None

        self.decoder_query_perturber = decoder_query_perturber
        self.box_pred_damping = None

        self.dec_layer_number = dec_layer_number
        if dec_layer_number is not None:
            assert isinstance(dec_layer_number, list)
            assert len(dec_layer_number) == num_layers

        self.dec_layer_dropout_prob = dec_layer_dropout_prob
        if dec_layer_dropout_prob is not None:
            assert isinstance(dec_layer_dropout_prob, list)
            assert len(dec_layer_dropout_prob) == num_layers
            for i in dec_layer_dropout_prob:
                assert 0.0 <= i <= 1.0

        self.rm_detach = None

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None,
                pos=None, refpoints_unsigmoid=None, level_start_index=None, spatial_shapes=None, valid_ratios=None):
        """tgt [nq, bs, d_model], memory / pos [hw, bs, d_model], refpoints_unsigmoid [nq, bs, 2 | 42], valid_ratios
        [bs, nlevel, 2]."""
        output = tgt
        intermediate = []
        reference_points = refpoints_unsigmoid.sigmoid() * 2 - 1
        ref_points = [reference_points]

        for layer_id, layer in enumerate(self.layers):
            if self.training and self.decoder_query_perturber is not None and layer_id != 0:
                reference_points = self.decoder_query_perturber(reference_points)

            if reference_points.shape[-1] not in (2, 42):
                raise AssertionError("reference_points must have 2 or 42 coordinates per query")
            # the points in every level's valid frame, for the cross-attention (:731-737), sequence-first as the layer takes them
            reference_points_input = decoder_reference_points(reference_points.transpose(0, 1), valid_ratios).transpose(0, 1)
            # ref_point_head(gen_sineembed_for_position(level 0 of the above)) (:738-746; query_scale is None: pos_scale = 1).
            # The table itself (the reference's query_sine_embed) is read by no 'sa' layer and is not passed on.
            query_pos = DF.query_pos(reference_points, valid_ratios, self.ref_point_head)

            dropflag = False
            if self.dec_layer_dropout_prob is not None:
                prob = random.random()
                if prob < self.dec_layer_dropout_prob[layer_id]:
                    dropflag = True
            if not dropflag:
                output = layer(tgt=output, tgt_query_pos=query_pos, tgt_query_sine_embed=None,
                               tgt_key_padding_mask=tgt_key_padding_mask, tgt_reference_points=reference_points_input,
                               memory=memory, memory_key_padding_mask=memory_key_padding_mask,
                               memory_level_start_index=level_start_index, memory_spatial_shapes=spatial_shapes, memory_pos=pos,
                               self_attn_mask=tgt_mask, cross_attn_mask=memory_mask)

            # iter update
            if self.key_embed is not None:
                cls_out = self.class_embed[layer_id](output)
                delta_key_unsig = self.key_embed[layer_id](output)
                delta_obj_key_unsig = self.obj_key_embed[layer_id](output)
                new_reference_points = DF.refine(reference_points, cls_out, delta_key_unsig, delta_obj_key_unsig, self.hand_classes)

                if self.dec_layer_number is not None and layer_id != self.num_layers - 1:
                    raise Exception('Not implemented')

                if self.rm_detach and 'dec' in self.rm_detach:
                    reference_points = new_reference_points
                else:
                    reference_points = new_reference_points.detach()
                if self.use_detached_boxes_dec_out:
                    ref_points.append(reference_points)
                else:
                    ref_points.append(new_reference_points)

            intermediate.append(add_layer_norm(output, None, self.norm))

        return [
            [itm_out.transpose(0, 1) for itm_out in intermediate],
            [itm_refpoint.transpose(0, 1) for itm_refpoint in ref_points]
        ]
