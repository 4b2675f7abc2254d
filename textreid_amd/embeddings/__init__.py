"""Embedding heads that sit on pooled encoder features (reference ``lib/models/embeddings/build.py:4-9``).
The MoCo head owns its encoders and is built by ``moco_head.head.build_moco_head`` instead."""
from .simple_head.head import build_simple_head


def build_embed(cfg, visual_out_channels, textual_out_channels):
    if cfg.MODEL.EMBEDDING.EMBED_HEAD == "simple":
        return build_simple_head(cfg, visual_out_channels, textual_out_channels)
    raise NotImplementedError("EMBED_HEAD=%r" % (cfg.MODEL.EMBEDDING.EMBED_HEAD,))
