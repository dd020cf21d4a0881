from .assembly_transformer import DeformableTransformer as AssemblyDeformableTransformer
from .assembly_transformer import DeformableTransformerDecoder as AssemblyDeformableTransformerDecoder
from .deformable_layers import (DeformableTransformerDecoder, DeformableTransformerDecoderLayer,
                                DeformableTransformerEncoder, DeformableTransformerEncoderLayer)
from .deformable_transformer import DeformableTransformer
from .detr import ArcticDeformableDETR, AssemblyDeformableDETR
from .dino import DINO, build_dino_model
from .dino_deformable_transformer import DeformableTransformer as DinoDeformableTransformer
from .dino_deformable_transformer import DeformableTransformerEncoderLayer as DinoDeformableTransformerEncoderLayer
from .dino_deformable_transformer import TransformerEncoder as DinoTransformerEncoder
from .dino_deformable_transformer import build_deformable_transformer as build_dino_deformable_transformer
from .dino_transformer import DeformableTransformerDecoderLayer as DinoDeformableTransformerDecoderLayer
from .dino_transformer import TransformerDecoder as DinoTransformerDecoder
from .ms_deform_attn import MSDeformAttn
from .smoothnet import ArcticSmoother, MotionSmoother, SmoothCriterion, Smoother, SmootherResBlock
from .swin import (BasicLayer, Joiner, Mlp, PatchEmbed, PatchMerging, PositionEmbeddingSine, SwinTransformer,
                   SwinTransformerBlock, WindowAttention, build_backbone, build_swin_transformer)

__all__ = ["MSDeformAttn", "DeformableTransformerEncoderLayer", "DeformableTransformerDecoderLayer",
           "DeformableTransformerEncoder", "DeformableTransformerDecoder", "DeformableTransformer",
           "AssemblyDeformableTransformer", "AssemblyDeformableTransformerDecoder",
           "ArcticDeformableDETR", "AssemblyDeformableDETR",
           "DinoDeformableTransformerDecoderLayer", "DinoTransformerDecoder",
           "DinoDeformableTransformer", "DinoTransformerEncoder", "DinoDeformableTransformerEncoderLayer",
           "build_dino_deformable_transformer", "DINO", "build_dino_model",
           "SmootherResBlock", "Smoother", "MotionSmoother", "ArcticSmoother", "SmoothCriterion",
           "Mlp", "WindowAttention", "SwinTransformerBlock", "PatchMerging", "BasicLayer", "PatchEmbed", "SwinTransformer",
           "build_swin_transformer", "PositionEmbeddingSine", "Joiner", "build_backbone"]
