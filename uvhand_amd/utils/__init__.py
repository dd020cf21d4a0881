from .denoising import (cdn_attention_mask, cdn_draws, cdn_group_arithmetic, dn_post_process, prepare_for_cdn,
                        prepare_for_cdn_composition)
from .transformer_inputs import (decoder_reference_points, encoder_reference_points, flatten_feature_levels,
                                 get_valid_ratio)

__all__ = ["flatten_feature_levels", "get_valid_ratio", "encoder_reference_points", "decoder_reference_points",
           "cdn_attention_mask", "prepare_for_cdn", "prepare_for_cdn_composition", "cdn_draws", "cdn_group_arithmetic",
           "dn_post_process"]
