"""``DeformableTransformer`` / ``TransformerEncoder`` / ``DeformableTransformerEncoderLayer`` of UVHand's DINO model
(models/dino/deformable_transformer.py:25-478, :481-625, :829-884) and ``build_deformable_transformer`` (:1068-1131), drop-in.
Exported from ``uvhand_amd.modules`` as ``DinoDeformableTransformer`` / ``DinoTransformerEncoder`` /
``DinoDeformableTransformerEncoderLayer`` / ``build_dino_deformable_transformer``.

Contract kept: the constructor signatures and defaults; the sub-module and parameter names in the reference's creation order
(``encoder, decoder, level_embed, tgt_embed, enc_output, enc_output_norm, two_stage_wh_embedding`` / ``refpoint_embed``), hence
the checkpoint keys; the same ``_reset_parameters``, so a construction under one ``torch.manual_seed`` gives a bit-identical
``state_dict``; ``get_valid_ratio``; ``forward(srcs, masks, refpoint_embed, pos_embeds, tgt, attn_mask=None)`` with the
reference's five-tuple ``(hs, references, hs_enc, ref_enc, init_box_proposal_unsig)``.  ``enc_out_class_embed`` /
``enc_out_bbox_embed`` start as ``None``; ``enc_out_class_embed``, ``enc_out_key_embed`` and ``enc_out_obj_key_embed`` are
attached from outside, as dino.py:208-220 does.  What every ``config/DINO/*.py`` sets is required (``deformable_encoder =
deformable_decoder = True``, ``learnable_tgt_init=True``, ``decoder_sa_type='sa'``, ``layer_share_type=None``);
``use_deformable_box_attn``, ``add_channel_attention`` and ``two_stage_keep_all_tokens=True`` (which reaches an unbound
``hs_enc`` in the reference, :453-457) raise ``NotImplementedError`` at construction; ``two_stage_type='no'`` constructs as the
reference does and raises its ``NotImplementedError`` in ``forward`` (:423-424).

``ref_enc`` carries no gradient, as in the reference: :372-373 rebind ``obj_kp`` / ``hand_kp`` to detached tensors before
:461-464 build ``ref_enc`` from them.  So the two keypoint heads, which are row-wise, only ever matter on the selected rows.

The two-stage block has two forms:

  * heads after selection — fp32 CUDA tensors outside autocast, ``MSDA_DINO_FUSED`` on, heads that are an ``nn.Linear`` or this
    package's ``MLP`` of plain ``nn.Linear`` layers without hooks: the class head on every row, ``select_queries_dino`` (HIP
    kernels for any number of rows per frame; one autograd node that carries the gradient of ``hs_enc`` to the encoder), the two
    keypoint heads on the Q selected rows under ``no_grad``, two ``torch.where``.  No host synchronisation;
  * the reference's structure — everything else: the heads on every row, ``torch.gather``, and the reference's boolean-mask
    assignments (:376-377) with their host synchronisations.

``two_stage_route`` (``None`` = the rule above, ``'selected'``, ``'reference'``) forces a form, for tests and measurements."""
import math
import random

import torch
from torch import nn

from ..functions import dino_func as DF
from ..functions import two_stage_func as TS
from ..functions.layernorm_func import add_layer_norm
from ..functions.linear_func import bracket_linear, fused_ffn
from ..utils.transformer_inputs import encoder_reference_points, flatten_feature_levels, level_tensors
from ..utils.transformer_inputs import get_valid_ratio as _valid_ratio
from .deformable_layers import _has_listener
from .detr import MLP
from .dino_transformer import DeformableTransformerDecoderLayer, TransformerDecoder, _get_activation_fn, _get_clones
from .ms_deform_attn import MSDeformAttn


class DeformableTransformerEncoderLayer(nn.Module):
    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4,
                 add_channel_attention=False, use_deformable_box_attn=False, box_attn_type='roi_align'):
        super().__init__()
        if use_deformable_box_attn:
            raise NotImplementedError("use_deformable_box_attn=True (MSDeformableBoxAttention) is not part of this package")
        if add_channel_attention:
            raise NotImplementedError("add_channel_attention=True (the 'dyrelu' activation) is not part of this package")
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation)
        self.dropout2 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout3 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)
        self.add_channel_attention = add_channel_attention

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, src):
        src2 = fused_ffn(src, self.linear1, self.activation, self.dropout2, self.linear2)
        return add_layer_norm(src, self.dropout3(src2), self.norm2)

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask=None):
        src2 = self.self_attn(self.with_pos_embed(src, pos), reference_points, src, spatial_shapes, level_start_index,
                              key_padding_mask)
        src = add_layer_norm(src, self.dropout1(src2), self.norm1)
        return self.forward_ffn(src)


class TransformerEncoder(nn.Module):
    def __init__(self, encoder_layer, num_layers, norm=None, d_model=256, num_queries=300, deformable_encoder=False,
                 enc_layer_share=False, enc_layer_dropout_prob=None, two_stage_type='no'):
        super().__init__()
        if not deformable_encoder:
            raise NotImplementedError("deformable_encoder=False is not built here (nor by the reference's transformer, :111-112)")
        if two_stage_type in ['enceachlayer', 'enclayer1']:
            raise NotImplementedError("two_stage_type=%r: per-layer encoder selection raises in the reference's forward (:598) "
                                      "and is not built here" % two_stage_type)
        if num_layers > 0:
            self.layers = _get_clones(encoder_layer, num_layers, layer_share=enc_layer_share)
        else:
            self.layers = []
        self.query_scale = None
        self.num_queries = num_queries
        self.deformable_encoder = deformable_encoder
        self.num_layers = num_layers
        self.norm = norm
        self.d_model = d_model
        self.enc_layer_dropout_prob = enc_layer_dropout_prob
        if enc_layer_dropout_prob is not None:
            assert isinstance(enc_layer_dropout_prob, list)
            assert len(enc_layer_dropout_prob) == num_layers
            for i in enc_layer_dropout_prob:
                assert 0.0 <= i <= 1.0
        self.two_stage_type = two_stage_type

    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device):
        return encoder_reference_points(spatial_shapes, valid_ratios, device)

    def forward(self, src, pos, spatial_shapes, level_start_index, valid_ratios, key_padding_mask, ref_token_index=None,
                ref_token_coord=None, level_hw=None):
        """src / pos [bs, sum(hi*wi), 256] -> (output, None, None), the reference's triple without per-layer selection.
        ``level_hw``: the levels' (H, W) as Python ints — given, the reference points are built without reading
        ``spatial_shapes`` back from the device."""
        assert ref_token_index is None
        output = src
        if self.num_layers > 0:
            reference_points = self.get_reference_points(level_hw if level_hw is not None else spatial_shapes, valid_ratios,
                                                         device=src.device)
        for layer_id, layer in enumerate(self.layers):
            dropflag = False
            if self.enc_layer_dropout_prob is not None:
                prob = random.random()
                if prob < self.enc_layer_dropout_prob[layer_id]:
                    dropflag = True
            if not dropflag:
                output = layer(src=output, pos=pos, reference_points=reference_points, spatial_shapes=spatial_shapes,
                               level_start_index=level_start_index, key_padding_mask=key_padding_mask)
        if self.norm is not None:
            output = add_layer_norm(output, None, self.norm)
        return output, None, None


def _plain_head(head):
    """An ``nn.Linear`` or this package's ``MLP`` of plain ``nn.Linear`` layers, nothing listening: a row-wise function."""
    if type(head) is nn.Linear:
        return not _has_listener(head)
    return (type(head) is MLP and all(type(l) is nn.Linear for l in head.layers)
            and not any(_has_listener(m) for m in head.modules()))


def inverse_sigmoid(x, eps=1e-5):
    return DF.inverse_sigmoid(x, eps)


class DeformableTransformer(nn.Module):
    hand_classes = (12, 13)                       # left / right hand in the ARCTIC label set (:354)

    def __init__(self, d_model=256, nhead=8, num_queries=300, num_encoder_layers=6, num_unicoder_layers=0, num_decoder_layers=6,
                 dim_feedforward=2048, dropout=0.0, activation="relu", normalize_before=False, return_intermediate_dec=False,
                 query_dim=4, num_patterns=0, modulate_hw_attn=False,
                 deformable_encoder=False, deformable_decoder=False, num_feature_levels=1, enc_n_points=4, dec_n_points=4,
                 use_deformable_box_attn=False, box_attn_type='roi_align',
                 learnable_tgt_init=False, decoder_query_perturber=None, add_channel_attention=False, add_pos_value=False,
                 random_refpoints_xy=False,
                 two_stage_type='no', two_stage_pat_embed=0, two_stage_add_query_num=0, two_stage_learn_wh=False,
                 two_stage_keep_all_tokens=False,
                 dec_layer_number=None, rm_enc_query_scale=True, rm_dec_query_scale=True, rm_self_attn_layers=None,
                 key_aware_type=None, layer_share_type=None, rm_detach=None, decoder_sa_type='ca', module_seq=['sa', 'ca', 'ffn'],
                 embed_init_tgt=False, use_detached_boxes_dec_out=False):
        super().__init__()
        self.num_feature_levels = num_feature_levels
        self.num_encoder_layers = num_encoder_layers
        self.num_unicoder_layers = num_unicoder_layers
        self.num_decoder_layers = num_decoder_layers
        self.deformable_encoder = deformable_encoder
        self.deformable_decoder = deformable_decoder
        self.two_stage_keep_all_tokens = two_stage_keep_all_tokens
        self.num_queries = num_queries
        self.random_refpoints_xy = random_refpoints_xy
        self.use_detached_boxes_dec_out = use_detached_boxes_dec_out
        assert query_dim == 4
        if use_deformable_box_attn:
            raise NotImplementedError("use_deformable_box_attn=True (MSDeformableBoxAttention) is not part of this package")
        if add_channel_attention:
            raise NotImplementedError("add_channel_attention=True (the 'dyrelu' activation) is not part of this package")
        if two_stage_keep_all_tokens:
            raise NotImplementedError("two_stage_keep_all_tokens=True leaves hs_enc unbound in the reference's forward (:453-457)")
        if num_feature_levels > 1:
            assert deformable_encoder, "only support deformable_encoder for num_feature_levels > 1"
        assert layer_share_type in [None, 'encoder', 'decoder', 'both']
        assert layer_share_type is None
        self.decoder_sa_type = decoder_sa_type
        assert decoder_sa_type in ['sa', 'ca_label', 'ca_content']

        if not deformable_encoder:
            raise NotImplementedError
        encoder_layer = DeformableTransformerEncoderLayer(d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead,
                                                          enc_n_points, add_channel_attention=add_channel_attention,
                                                          use_deformable_box_attn=use_deformable_box_attn,
                                                          box_attn_type=box_attn_type)
        encoder_norm = nn.LayerNorm(d_model) if normalize_before else None
        self.encoder = TransformerEncoder(encoder_layer, num_encoder_layers, encoder_norm, d_model=d_model, num_queries=num_queries,
                                          deformable_encoder=deformable_encoder, enc_layer_share=False,
                                          two_stage_type=two_stage_type)

        if not deformable_decoder:
            raise NotImplementedError
        decoder_layer = DeformableTransformerDecoderLayer(d_model, dim_feedforward, dropout, activation, num_feature_levels, nhead,
                                                          dec_n_points, use_deformable_box_attn=use_deformable_box_attn,
                                                          box_attn_type=box_attn_type, key_aware_type=key_aware_type,
                                                          decoder_sa_type=decoder_sa_type, module_seq=module_seq)
        decoder_norm = nn.LayerNorm(d_model)
        self.decoder = TransformerDecoder(decoder_layer, num_decoder_layers, decoder_norm, return_intermediate=return_intermediate_dec,
                                          d_model=d_model, query_dim=query_dim, modulate_hw_attn=modulate_hw_attn,
                                          num_feature_levels=num_feature_levels, deformable_decoder=deformable_decoder,
                                          decoder_query_perturber=decoder_query_perturber, dec_layer_number=dec_layer_number,
                                          rm_dec_query_scale=rm_dec_query_scale, dec_layer_share=False,
                                          use_detached_boxes_dec_out=use_detached_boxes_dec_out)

        self.d_model = d_model
        self.nhead = nhead
        self.dec_layers = num_decoder_layers
        self.num_queries = num_queries
        self.num_patterns = num_patterns
        if not isinstance(num_patterns, int):
            self.num_patterns = 0

        if num_feature_levels > 1:
            if self.num_encoder_layers > 0:
                self.level_embed = nn.Parameter(torch.Tensor(num_feature_levels, d_model))
            else:
                self.level_embed = None

        self.learnable_tgt_init = learnable_tgt_init
        assert learnable_tgt_init, "why not learnable_tgt_init"
        self.embed_init_tgt = embed_init_tgt
        if (two_stage_type != 'no' and embed_init_tgt) or (two_stage_type == 'no'):
            self.tgt_embed = nn.Embedding(self.num_queries, d_model)
            nn.init.normal_(self.tgt_embed.weight.data)
        else:
            self.tgt_embed = None

        self.two_stage_type = two_stage_type
        self.two_stage_pat_embed = two_stage_pat_embed
        self.two_stage_add_query_num = two_stage_add_query_num
        self.two_stage_learn_wh = two_stage_learn_wh
        assert two_stage_type in ['no', 'standard'], "unknown param {} of two_stage_type".format(two_stage_type)
        if two_stage_type == 'standard':
            self.enc_output = nn.Linear(d_model, d_model)
            self.enc_output_norm = nn.LayerNorm(d_model)
            if two_stage_pat_embed > 0:
                self.pat_embed_for_2stage = nn.Parameter(torch.Tensor(two_stage_pat_embed, d_model))
                nn.init.normal_(self.pat_embed_for_2stage)
            if two_stage_add_query_num > 0:
                self.tgt_embed = nn.Embedding(self.two_stage_add_query_num, d_model)
            if two_stage_learn_wh:
                self.two_stage_wh_embedding = nn.Embedding(1, 40)
            else:
                self.two_stage_wh_embedding = None
        if two_stage_type == 'no':
            self.init_ref_points(num_queries)

        self.enc_out_class_embed = None
        self.enc_out_bbox_embed = None

        self.dec_layer_number = dec_layer_number
        if dec_layer_number is not None:
            if self.two_stage_type != 'no' or num_patterns == 0:
                assert dec_layer_number[0] == num_queries, \
                    f"dec_layer_number[0]({dec_layer_number[0]}) != num_queries({num_queries})"
            else:
                assert dec_layer_number[0] == num_queries * num_patterns, \
                    f"dec_layer_number[0]({dec_layer_number[0]}) != num_queries({num_queries}) * num_patterns({num_patterns})"

        self._reset_parameters()

        self.rm_self_attn_layers = rm_self_attn_layers
        if rm_self_attn_layers is not None:
            for lid, dec_layer in enumerate(self.decoder.layers):
                if lid in rm_self_attn_layers:
                    dec_layer.rm_self_attn_modules()

        self.rm_detach = rm_detach
        if self.rm_detach:
            assert isinstance(rm_detach, list)
            assert any([i in ['enc_ref', 'enc_tgt', 'dec'] for i in rm_detach])
        self.decoder.rm_detach = rm_detach
        self.two_stage_route = None               # None | 'selected' | 'reference' (the module's docstring)
        self._level_tensors = {}                  # (levels' (H, W), device) -> (spatial_shapes, level_start_index)

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, MSDeformAttn):
                m._reset_parameters()
        if self.num_feature_levels > 1 and self.level_embed is not None:
            nn.init.normal_(self.level_embed)
        if self.two_stage_learn_wh:
            nn.init.constant_(self.two_stage_wh_embedding.weight, math.log(0.05 / (1 - 0.05)))

    def get_valid_ratio(self, mask):
        return _valid_ratio(mask)

    def init_ref_points(self, use_num_queries):
        self.refpoint_embed = nn.Embedding(use_num_queries, 4)
        if self.random_refpoints_xy:
            self.refpoint_embed.weight.data[:, :2].uniform_(0, 1)
            self.refpoint_embed.weight.data[:, :2] = inverse_sigmoid(self.refpoint_embed.weight.data[:, :2])
            self.refpoint_embed.weight.data[:, :2].requires_grad = False

    # ---- the two-stage block (:318-403) ---------------------------------------------------------------------------------
    def heads_after_selection(self, enc_class, output_memory, output_proposals):
        """The rule of the module's docstring: the kernels apply and the three heads are plain row-wise functions."""
        if self.two_stage_route is not None:
            return self.two_stage_route == 'selected'
        return (DF.select_fusable(enc_class, output_memory, output_proposals, self.num_queries)
                and all(_plain_head(h) for h in (self.enc_out_class_embed, self.enc_out_key_embed, self.enc_out_obj_key_embed)))

    def _select_reference(self, enc_class, output_memory, output_proposals):
        """:341-387 as the reference writes them: both keypoint heads on every row, gathers, boolean-mask assignments."""
        hand_all = self.enc_out_key_embed(output_memory)
        obj_all = self.enc_out_obj_key_embed(output_memory)
        hand_all[..., 0::2] += output_proposals[..., 0::2]
        hand_all[..., 1::2] += output_proposals[..., 1::2]
        obj_all[..., 0::2] += output_proposals[..., 0::2]
        obj_all[..., 1::2] += output_proposals[..., 1::2]
        topk_proposals = torch.topk(enc_class.max(-1)[0], self.num_queries, dim=1)[1]
        class_indices = torch.gather(enc_class.argmax(dim=-1), 1, topk_proposals)
        hand_idx = (class_indices == self.hand_classes[0]) + (class_indices == self.hand_classes[1])
        obj_idx = ~hand_idx * (class_indices != 0)
        hand_idx = hand_idx.unsqueeze(-1).repeat(1, 1, 42)
        obj_idx = obj_idx.unsqueeze(-1).repeat(1, 1, 42)
        index = topk_proposals.unsqueeze(-1).repeat(1, 1, 42)
        obj_kp = torch.gather(obj_all, 1, index).detach()
        hand_kp = torch.gather(hand_all, 1, index).detach()
        # (the proposals are fp32 whatever memory's dtype when there are no learned offsets, :35-45; the assignments want one dtype)
        init_box_proposal_unsig = torch.gather(output_proposals, 1, index).detach().to(obj_kp.dtype)
        init_box_proposal_unsig[obj_idx] = obj_kp[obj_idx]
        init_box_proposal_unsig[hand_idx] = hand_kp[hand_idx]
        tgt_undetach = torch.gather(output_memory, 1, topk_proposals.unsqueeze(-1).repeat(1, 1, self.d_model))
        return topk_proposals, tgt_undetach, obj_kp, hand_kp, init_box_proposal_unsig

    def _select_rows(self, enc_class, output_memory, output_proposals):
        """The same values with the keypoint heads on the Q selected rows only and no mask assignment."""
        topk_proposals, tgt_undetach, prop_sel, code = DF.select_queries_dino(enc_class, output_memory, output_proposals,
                                                                              self.num_queries, self.hand_classes)
        with torch.no_grad():
            rows = tgt_undetach.detach()
            hand_kp = self.enc_out_key_embed(rows) + prop_sel
            obj_kp = self.enc_out_obj_key_embed(rows) + prop_sel
            code = code.unsqueeze(-1)
            init_box_proposal_unsig = torch.where(code == 2, hand_kp, torch.where(code == 1, obj_kp, prop_sel))
        return topk_proposals, tgt_undetach, obj_kp, hand_kp, init_box_proposal_unsig

    def two_stage_block(self, memory, mask_flatten, level_hw):
        """:318-387: (topk_proposals [bs, nq], tgt_undetach [bs, nq, d_model], obj_kp, hand_kp, init_box_proposal_unsig
        [bs, nq, 42] — the last three detached) from the encoder's output, its padding mask and the levels' (H, W)."""
        # the learned offsets reach the loss through detached tensors only (:371-373): no gradient, as in the reference
        input_hw = self.two_stage_wh_embedding.weight[0].detach() if self.two_stage_learn_wh else None
        output_memory, output_proposals = TS.encoder_output_proposals(memory, mask_flatten, level_hw, input_hw)
        output_memory = add_layer_norm(bracket_linear(output_memory, self.enc_output), None, self.enc_output_norm)
        enc_outputs_class_unselected = self.enc_out_class_embed(output_memory)
        select = (self._select_rows if self.heads_after_selection(enc_outputs_class_unselected, output_memory, output_proposals)
                  else self._select_reference)
        return select(enc_outputs_class_unselected, output_memory, output_proposals)

    def forward(self, srcs, masks, refpoint_embed, pos_embeds, tgt, attn_mask=None):
        """srcs / pos_embeds: lists of [bs, c, hi, wi]; masks: list of [bs, hi, wi]; refpoint_embed [bs, num_dn, 42] and tgt
        [bs, num_dn, d_model], or None.  ``self.last_topk_proposals`` keeps the selected rows [bs, nq] of the call."""
        if self.two_stage_type != 'standard':
            raise NotImplementedError("unknown two_stage_type {}".format(self.two_stage_type))
        level_hw = [(int(s.shape[2]), int(s.shape[3])) for s in srcs]
        # the level tensors of a pyramid are made once and handed to every later call: no host-to-device copy per step, and
        # MSDeformAttn's check of the shapes (once per tensor) stays out of the steady state
        key = (tuple(level_hw), srcs[0].device)
        if key not in self._level_tensors:
            self._level_tensors[key] = level_tensors(level_hw, srcs[0].device)
        level_embed = self.level_embed if self.num_feature_levels > 1 else None
        (src_flatten, mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index,
         valid_ratios) = flatten_feature_levels(srcs, masks, pos_embeds, level_embed, pyramid=self._level_tensors[key])
        bs = src_flatten.shape[0]

        memory, _, _ = self.encoder(src_flatten, pos=lvl_pos_embed_flatten, level_start_index=level_start_index,
                                    spatial_shapes=spatial_shapes, valid_ratios=valid_ratios, key_padding_mask=mask_flatten,
                                    level_hw=level_hw)

        topk_proposals, tgt_undetach, obj_kp, hand_kp, init_box_proposal_unsig = self.two_stage_block(memory, mask_flatten, level_hw)
        self.last_topk_proposals = topk_proposals
        refpoint_embed_ = init_box_proposal_unsig
        if self.embed_init_tgt:
            tgt_ = self.tgt_embed.weight[:, None, :].repeat(1, bs, 1).transpose(0, 1)
        else:
            tgt_ = tgt_undetach.detach()
        if refpoint_embed is not None:
            refpoint_embed = torch.cat([refpoint_embed, refpoint_embed_], dim=1)
            tgt = torch.cat([tgt, tgt_], dim=1)
        else:
            refpoint_embed, tgt = refpoint_embed_, tgt_

        hs, references = self.decoder(tgt=tgt.transpose(0, 1), memory=memory.transpose(0, 1), memory_key_padding_mask=mask_flatten,
                                      pos=lvl_pos_embed_flatten.transpose(0, 1), refpoints_unsigmoid=refpoint_embed.transpose(0, 1),
                                      level_start_index=level_start_index, spatial_shapes=spatial_shapes, valid_ratios=valid_ratios,
                                      tgt_mask=attn_mask)

        hs_enc = tgt_undetach.unsqueeze(0)
        ref_enc = [(obj_kp.sigmoid() * 2 - 1).unsqueeze(0), (hand_kp.sigmoid() * 2 - 1).unsqueeze(0)]
        return hs, references, hs_enc, ref_enc, init_box_proposal_unsig


def build_deformable_transformer(args):
    """models/dino/deformable_transformer.py:1068-1131: the same arguments read off ``args``."""
    decoder_query_perturber = None
    if args.decoder_layer_noise:
        raise NotImplementedError("decoder_layer_noise=True (RandomBoxPerturber) is not part of this package")
    use_detached_boxes_dec_out = getattr(args, "use_detached_boxes_dec_out", False)
    return DeformableTransformer(
        d_model=args.hidden_dim, dropout=args.dropout, nhead=args.nheads, num_queries=args.num_queries,
        dim_feedforward=args.dim_feedforward, num_encoder_layers=args.enc_layers, num_unicoder_layers=args.unic_layers,
        num_decoder_layers=args.dec_layers, normalize_before=args.pre_norm, return_intermediate_dec=True, query_dim=args.query_dim,
        activation=args.transformer_activation, num_patterns=args.num_patterns, modulate_hw_attn=True,
        deformable_encoder=True, deformable_decoder=True, num_feature_levels=args.num_feature_levels,
        enc_n_points=args.enc_n_points, dec_n_points=args.dec_n_points, use_deformable_box_attn=args.use_deformable_box_attn,
        box_attn_type=args.box_attn_type, learnable_tgt_init=True, decoder_query_perturber=decoder_query_perturber,
        add_channel_attention=args.add_channel_attention, add_pos_value=args.add_pos_value,
        random_refpoints_xy=args.random_refpoints_xy, two_stage_type=args.two_stage_type,
        two_stage_pat_embed=args.two_stage_pat_embed, two_stage_add_query_num=args.two_stage_add_query_num,
        two_stage_learn_wh=True, two_stage_keep_all_tokens=args.two_stage_keep_all_tokens,
        dec_layer_number=args.dec_layer_number, rm_self_attn_layers=None, key_aware_type=None, layer_share_type=None,
        rm_detach=None, decoder_sa_type=args.decoder_sa_type, module_seq=args.decoder_module_seq,
        embed_init_tgt=args.embed_init_tgt, use_detached_boxes_dec_out=use_detached_boxes_dec_out)
