"""Drop-in DINO model class (models/dino/dino.py:46-426) and ``build_dino_model`` (build_dino :855-903, the model only).

Constructor signature and defaults, sub-module names and creation order, parameter init (``_reset_parameters`` included), the
sharing of the class / keypoint heads with ``transformer.decoder`` and ``transformer.enc_out_*`` under the four ``*_share``
flags, ``init_ref_points``, the ``label_embedding`` handling, the assertions and the output dict are the reference's: one
``torch.manual_seed`` builds a bit-identical ``state_dict`` and a reference checkpoint loads with ``strict=True``.  ``backbone``
and ``transformer`` are injected; the transformer is any module with the reference's five-tuple contract
(``DinoDeformableTransformer`` is the intended one).

What runs where: the pyramid comes from ``modules.detr._backbone_inputs`` (the neck node), the denoising queries from
``utils.prepare_for_cdn`` / ``utils.dn_post_process``, and everything after the transformer is ``heads``, built on
``functions.heads_func.dino_heads``: on CUDA fp32 three forward and at most six backward HIP launches for every head of every
decoder layer, with the gradient to the undetached references ("look forward twice") from the library's own kernel.

Left out: ``build_backbone``, the criterion wiring of ``build_dino``, ``DETRsegm`` and ``PostProcess`` (it reads
``pred_boxes``, which this model never emits)."""
import copy
import math

import torch
from torch import nn

from ..functions.heads_func import dino_heads, inverse_sigmoid
from ..utils.denoising import dn_post_process, prepare_for_cdn
from .detr import MLP, _backbone_inputs
from .dino_deformable_transformer import build_deformable_transformer

__all__ = ["DINO", "build_dino_model"]


class DINO(nn.Module):
    """models/dino/dino.py DINO."""

    def __init__(self, backbone, transformer, num_classes, num_queries,
                 aux_loss=False, iter_update=False,
                 query_dim=2,
                 random_refpoints_xy=False,
                 fix_refpoints_hw=-1,
                 num_feature_levels=1,
                 nheads=8,
                 # two stage
                 two_stage_type='no',  # ['no', 'standard']
                 two_stage_add_query_num=0,
                 dec_pred_class_embed_share=True,
                 dec_pred_bbox_embed_share=True,
                 two_stage_class_embed_share=True,
                 two_stage_bbox_embed_share=True,
                 decoder_sa_type='sa',
                 num_patterns=0,
                 dn_number=100,
                 dn_box_noise_scale=0.4,
                 dn_label_noise_ratio=0.5,
                 dn_labelbook_size=100,
                 ):
        super().__init__()
        self.num_queries = num_queries
        self.transformer = transformer
        self.num_classes = num_classes
        self.hidden_dim = hidden_dim = transformer.d_model
        self.num_feature_levels = num_feature_levels
        self.nheads = nheads
        self.label_enc = nn.Embedding(dn_labelbook_size + 1, hidden_dim)

        # setting query dim
        self.query_dim = query_dim
        assert query_dim == 4
        self.random_refpoints_xy = random_refpoints_xy
        self.fix_refpoints_hw = fix_refpoints_hw

        # for dn training
        self.num_patterns = num_patterns
        self.dn_number = dn_number
        self.dn_box_noise_scale = dn_box_noise_scale
        self.dn_label_noise_ratio = dn_label_noise_ratio
        self.dn_labelbook_size = dn_labelbook_size

        # prepare input projection layers
        if num_feature_levels > 1:
            num_backbone_outs = len(backbone.num_channels)
            input_proj_list = []
            for _ in range(num_backbone_outs):
                in_channels = backbone.num_channels[_]
                input_proj_list.append(nn.Sequential(
                    nn.Conv2d(in_channels, hidden_dim, kernel_size=1),
                    nn.GroupNorm(32, hidden_dim),
                ))
            for _ in range(num_feature_levels - num_backbone_outs):
                input_proj_list.append(nn.Sequential(
                    nn.Conv2d(in_channels, hidden_dim, kernel_size=3, stride=2, padding=1),
                    nn.GroupNorm(32, hidden_dim),
                ))
                in_channels = hidden_dim
            self.input_proj = nn.ModuleList(input_proj_list)
        else:
            assert two_stage_type == 'no', "two_stage_type should be no if num_feature_levels=1 !!!"
            self.input_proj = nn.ModuleList([
                nn.Sequential(
                    nn.Conv2d(backbone.num_channels[-1], hidden_dim, kernel_size=1),
                    nn.GroupNorm(32, hidden_dim),
                )])

        self.backbone = backbone
        self.aux_loss = aux_loss
        self.box_pred_damping = None

        self.iter_update = iter_update
        assert iter_update, "Why not iter_update?"

        # prepare pred layers
        self.dec_pred_class_embed_share = dec_pred_class_embed_share
        self.dec_pred_bbox_embed_share = dec_pred_bbox_embed_share
        # prepare class & keypoint embed
        _class_embed = nn.Linear(hidden_dim, num_classes)
        _key_embed = MLP(hidden_dim, hidden_dim, 42, 3)
        _obj_key_embed = MLP(hidden_dim, hidden_dim, 42, 3)
        _mano_pose_embed = nn.Linear(hidden_dim, 48)
        _mano_beta_embed = nn.Linear(hidden_dim, 10)
        _hand_cam = nn.Linear(hidden_dim, 3)
        _obj_cam = nn.Linear(hidden_dim, 3)
        _obj_rot = nn.Linear(hidden_dim, 3)
        _obj_rad = nn.Linear(hidden_dim, 1)

        # init the two embed layers
        prior_prob = 0.01
        bias_value = -math.log((1 - prior_prob) / prior_prob)
        _class_embed.bias.data = torch.ones(self.num_classes) * bias_value
        nn.init.constant_(_key_embed.layers[-1].weight.data, 0)
        nn.init.constant_(_key_embed.layers[-1].bias.data, 0)
        nn.init.constant_(_obj_key_embed.layers[-1].weight.data, 0)
        nn.init.constant_(_obj_key_embed.layers[-1].bias.data, 0)

        for lin in (_mano_pose_embed, _mano_beta_embed, _hand_cam, _obj_cam, _obj_rot, _obj_rad):
            nn.init.xavier_uniform_(lin.weight, gain=1)
            nn.init.constant_(lin.bias.data, 0)

        n_dec = transformer.num_decoder_layers
        if dec_pred_bbox_embed_share:
            key_embed_layerlist = [_key_embed for i in range(n_dec)]
            obj_key_embed_layerlist = [_obj_key_embed for i in range(n_dec)]
        else:
            key_embed_layerlist = [copy.deepcopy(_key_embed) for i in range(n_dec)]
            obj_key_embed_layerlist = [copy.deepcopy(_obj_key_embed) for i in range(n_dec)]
        if dec_pred_class_embed_share:
            class_embed_layerlist = [_class_embed for i in range(n_dec)]
            mano_pose_embed_layerlist = [_mano_pose_embed for i in range(n_dec)]
            mano_beta_embed_layerlist = [_mano_beta_embed for i in range(n_dec)]
            hand_cam_layerlist = [_hand_cam for i in range(n_dec)]
            obj_cam_layerlist = [_obj_cam for i in range(n_dec)]
            obj_rot_layerlist = [_obj_rot for i in range(n_dec)]
            obj_rad_layerlist = [_obj_rad for i in range(n_dec)]
        else:
            raise Exception('Not implemented.')
        self.class_embed = nn.ModuleList(class_embed_layerlist)
        self.key_embed = nn.ModuleList(key_embed_layerlist)
        self.obj_key_embed = nn.ModuleList(obj_key_embed_layerlist)
        self.mano_pose_embed = nn.ModuleList(mano_pose_embed_layerlist)
        self.mano_beta_embed = nn.ModuleList(mano_beta_embed_layerlist)
        self.hand_cam = nn.ModuleList(hand_cam_layerlist)
        self.obj_cam = nn.ModuleList(obj_cam_layerlist)
        self.obj_rot = nn.ModuleList(obj_rot_layerlist)
        self.obj_rad = nn.ModuleList(obj_rad_layerlist)
        self.transformer.decoder.class_embed = self.class_embed
        self.transformer.decoder.key_embed = self.key_embed
        self.transformer.decoder.obj_key_embed = self.obj_key_embed

        # two stage
        self.two_stage_type = two_stage_type
        self.two_stage_add_query_num = two_stage_add_query_num
        assert two_stage_type in ['no', 'standard'], "unknown param {} of two_stage_type".format(two_stage_type)
        if two_stage_type != 'no':
            if two_stage_bbox_embed_share:
                assert dec_pred_class_embed_share and dec_pred_bbox_embed_share
                self.transformer.enc_out_key_embed = _key_embed
                self.transformer.enc_out_obj_key_embed = _obj_key_embed
            else:
                self.transformer.enc_out_key_embed = copy.deepcopy(_key_embed)
                self.transformer.enc_out_obj_key_embed = copy.deepcopy(_obj_key_embed)
            if two_stage_class_embed_share:
                assert dec_pred_class_embed_share and dec_pred_bbox_embed_share
                self.transformer.enc_out_class_embed = _class_embed
            else:
                self.transformer.enc_out_class_embed = copy.deepcopy(_class_embed)

            self.refpoint_embed = None
            if self.two_stage_add_query_num > 0:
                self.init_ref_points(two_stage_add_query_num)

        self.decoder_sa_type = decoder_sa_type
        assert decoder_sa_type in ['sa', 'ca_label', 'ca_content']
        if decoder_sa_type == 'ca_label':
            self.label_embedding = nn.Embedding(num_classes, hidden_dim)
            for layer in self.transformer.decoder.layers:
                layer.label_embedding = self.label_embedding
        else:
            for layer in self.transformer.decoder.layers:
                layer.label_embedding = None
            self.label_embedding = None

        self._reset_parameters()

    def _reset_parameters(self):
        # init input_proj
        for proj in self.input_proj:
            nn.init.xavier_uniform_(proj[0].weight, gain=1)
            nn.init.constant_(proj[0].bias, 0)

    def init_ref_points(self, use_num_queries):
        self.refpoint_embed = nn.Embedding(use_num_queries, self.query_dim)
        if self.random_refpoints_xy:
            self.refpoint_embed.weight.data[:, :2].uniform_(0, 1)
            self.refpoint_embed.weight.data[:, :2] = inverse_sigmoid(self.refpoint_embed.weight.data[:, :2])
            self.refpoint_embed.weight.data[:, :2].requires_grad = False

        if self.fix_refpoints_hw > 0:
            print("fix_refpoints_hw: {}".format(self.fix_refpoints_hw))
            assert self.random_refpoints_xy
            self.refpoint_embed.weight.data[:, 2:] = self.fix_refpoints_hw
            self.refpoint_embed.weight.data[:, 2:] = inverse_sigmoid(self.refpoint_embed.weight.data[:, 2:])
            self.refpoint_embed.weight.data[:, 2:].requires_grad = False
        elif int(self.fix_refpoints_hw) == -1:
            pass
        elif int(self.fix_refpoints_hw) == -2:
            print('learn a shared h and w')
            assert self.random_refpoints_xy
            self.refpoint_embed = nn.Embedding(use_num_queries, 2)
            self.refpoint_embed.weight.data[:, :2].uniform_(0, 1)
            self.refpoint_embed.weight.data[:, :2] = inverse_sigmoid(self.refpoint_embed.weight.data[:, :2])
            self.refpoint_embed.weight.data[:, :2].requires_grad = False
            self.hw_embed = nn.Embedding(1, 1)
        else:
            raise NotImplementedError('Unknown fix_refpoints_hw {}'.format(self.fix_refpoints_hw))

    def forward(self, samples, targets=None, packed=None):
        """samples: a NestedTensor, or a list / batch of images.  targets: the reference's dict (per-frame ``labels`` lists,
        ``keypoints`` tensors) or None.  packed: the ``PackedTargets`` already made of the same targets (``prepare_for_cdn``
        then copies nothing to the device); not a reference argument.  Returns the reference's output dict (:360-398)."""
        srcs, masks, poss = _backbone_inputs(self, samples, random_mask=False)

        if self.dn_number > 0 or targets is not None:
            input_query_label, input_query_bbox, attn_mask, dn_meta = prepare_for_cdn(
                dn_args=(targets, self.dn_number, self.dn_label_noise_ratio, self.dn_box_noise_scale),
                training=self.training, num_queries=self.num_queries, num_classes=self.num_classes,
                hidden_dim=self.hidden_dim, label_enc=self.label_enc, packed=packed)
        else:
            assert targets is None
            input_query_bbox = input_query_label = attn_mask = dn_meta = None

        hs, reference, hs_enc, ref_enc, init_box_proposal = self.transformer(srcs, masks, input_query_bbox, poss,
                                                                             input_query_label, attn_mask)
        # In case num object=0
        hs[0] += self.label_enc.weight[0, 0] * 0.0
        return self.heads(hs, reference, hs_enc, ref_enc, dn_meta)

    def heads(self, hs, reference, hs_enc, ref_enc, dn_meta):
        """Everything the reference's forward does after the transformer (:325-400).  hs: the decoder's per-layer outputs
        [N, Lq, C]; reference: its n_dec + 1 reference points [N, Lq, 42], of which all but the first carry a gradient."""
        shared = [self.mano_pose_embed[0], self.mano_beta_embed[0], self.hand_cam[0], self.obj_cam[0], self.obj_rot[0],
                  self.obj_rad[0]]
        outputs_class, (outputs_hand_coord_list, outputs_obj_coord_list), \
            (outputs_mano_pose, outputs_mano_beta, outputs_hand_cam, outputs_obj_cam, outputs_obj_rot, outputs_obj_rad) = \
            dino_heads(hs, reference[:-1], self.class_embed, self.key_embed, self.obj_key_embed, shared)

        outputs_mano_param = [outputs_mano_pose, outputs_mano_beta]
        outputs_cam_param = [outputs_hand_cam, outputs_obj_cam]
        outputs_obj_param = [outputs_obj_rad, outputs_obj_rot]

        if self.dn_number > 0 and dn_meta is not None:
            outputs_class, outputs_hand_coord_list, outputs_obj_coord_list, outputs_mano_param, outputs_cam_param, \
                outputs_obj_param = dn_post_process(
                    outputs_class, outputs_hand_coord_list, outputs_obj_coord_list,
                    outputs_mano_param, outputs_cam_param, outputs_obj_param,
                    dn_meta, self.aux_loss, self._set_aux_loss)
        out = {
            'pred_logits': outputs_class[-1], 'pred_hand_key': outputs_hand_coord_list[-1],
            'pred_obj_key': outputs_obj_coord_list[-1],
            'pred_mano_params': [outputs_mano_param[0][-1], outputs_mano_param[1][-1]],
            'pred_cams': [outputs_cam_param[0][-1], outputs_cam_param[1][-1]],
            'pred_obj_params': [outputs_obj_param[0][-1], outputs_obj_param[1][-1]],
        }
        if self.aux_loss:
            out['aux_outputs'] = self._set_aux_loss(
                outputs_class, outputs_hand_coord_list, outputs_obj_coord_list,
                outputs_mano_param, outputs_obj_param, outputs_cam_param)

        # for encoder output
        if hs_enc is not None:
            # :376-378: the first of ref_enc goes out as pred_hand_key, the second as pred_obj_key
            interm_obj, interm_hand = ref_enc
            interm_class = self.transformer.enc_out_class_embed(hs_enc[-1])
            out['interm_outputs'] = {'pred_logits': interm_class, 'pred_hand_key': interm_obj[-1],
                                     'pred_obj_key': interm_hand[-1]}

            # :382-396 read enc_bbox_embed / enc_class_embed, which the reference never creates: kept as its lines, so it
            # fails the same way, and only a transformer that returns more than one hs_enc layer gets here
            if hs_enc.shape[0] > 1:
                enc_outputs_coord = []
                enc_outputs_class = []
                for layer_id, (layer_box_embed, layer_class_embed, layer_hs_enc, layer_ref_enc) in enumerate(
                        zip(self.enc_bbox_embed, self.enc_class_embed, hs_enc[:-1], ref_enc[:-1])):
                    layer_enc_delta_unsig = layer_box_embed(layer_hs_enc)
                    layer_enc_outputs_coord_unsig = layer_enc_delta_unsig + inverse_sigmoid(layer_ref_enc)
                    layer_enc_outputs_coord = layer_enc_outputs_coord_unsig.sigmoid() * 2 - 1

                    layer_enc_outputs_class = layer_class_embed(layer_hs_enc)
                    enc_outputs_coord.append(layer_enc_outputs_coord)
                    enc_outputs_class.append(layer_enc_outputs_class)

                out['enc_outputs'] = [
                    {'pred_logits': a, 'pred_boxes': b} for a, b in zip(enc_outputs_class, enc_outputs_coord)
                ]

        out['dn_meta'] = dn_meta
        return out

    @torch.jit.unused
    def _set_aux_loss(self, outputs_class, hand_coord, obj_coord, outputs_mano_params, outputs_obj_params, outputs_cams):
        return [
            {
                'pred_logits': c, 'pred_hand_key': hk, 'pred_obj_key': ok,
                'pred_mano_params': [s, p], 'pred_obj_params': [ra, ro], 'pred_cams': [hc, oc]
            }
            for c, hk, ok, s, p, ra, ro, hc, oc in zip(
                outputs_class[:-1], hand_coord[:-1], obj_coord[:-1],
                outputs_mano_params[0][:-1], outputs_mano_params[1][:-1],
                outputs_obj_params[0][:-1], outputs_obj_params[1][:-1],
                outputs_cams[0][:-1], outputs_cams[1][:-1])
        ]


def build_dino_model(args, backbone):
    """The model of build_dino (models/dino/dino.py:855-903) over an injected backbone: the transformer from
    ``build_dino_deformable_transformer(args)`` and ``DINO`` with the reference's arguments.  The criterion, the
    post-processors and ``DETRsegm`` are not built here."""
    num_classes = args.num_classes
    transformer = build_deformable_transformer(args)
    try:                                            # :862-867: both attributes, or the default
        args.match_unstable_error
        dn_labelbook_size = args.dn_labelbook_size
    except AttributeError:
        dn_labelbook_size = num_classes
    return DINO(
        backbone,
        transformer,
        num_classes=num_classes,
        num_queries=args.num_queries,
        aux_loss=True,
        iter_update=True,
        query_dim=4,
        random_refpoints_xy=args.random_refpoints_xy,
        fix_refpoints_hw=args.fix_refpoints_hw,
        num_feature_levels=args.num_feature_levels,
        nheads=args.nheads,
        dec_pred_class_embed_share=getattr(args, "dec_pred_class_embed_share", True),
        dec_pred_bbox_embed_share=getattr(args, "dec_pred_bbox_embed_share", True),
        # two stage
        two_stage_type=args.two_stage_type,
        two_stage_bbox_embed_share=args.two_stage_bbox_embed_share,
        two_stage_class_embed_share=args.two_stage_class_embed_share,
        decoder_sa_type=args.decoder_sa_type,
        num_patterns=args.num_patterns,
        dn_number=args.dn_number if args.use_dn else 0,
        dn_box_noise_scale=args.dn_box_noise_scale,
        dn_label_noise_ratio=args.dn_label_noise_ratio,
        dn_labelbook_size=dn_labelbook_size,
    )
