"""Simple embedding head on the HIP kernel library (the baseline configs' ``EMBED_HEAD: 'simple'``).

Operator surface of the reference ``lib/models/embeddings/simple_head/head.py`` (``SimpleHead`` :6-47,
``build_simple_head`` :50): one Linear per modality onto the joint space; ``forward(visual_feature,
textual_feature, captions)`` returns ``(None, {"instance_loss", "global_align_loss"})`` in training and
``([v_embed, t_embed], None)`` in eval.  Same parameter names and shapes, so reference checkpoints load.
Unlike the MoCo head it owns no encoders: ``textreid_amd.model.Model`` runs them (its "normal" branch).
"""
import torch.nn as nn

from ... import losses
from .loss import make_loss_evaluator


class SimpleHead(nn.Module):
    def __init__(self, cfg, visual_size, textual_size):
        super().__init__()
        self.embed_size = cfg.MODEL.EMBEDDING.FEATURE_SIZE
        # construction order = the reference's draw order from the global RNG: the two Linears, then the projection
        self.visual_embed_layer = nn.Linear(visual_size, self.embed_size)
        self.textual_embed_layer = nn.Linear(textual_size, self.embed_size)
        self.loss_evaluator = make_loss_evaluator(cfg)
        self._init_weight()

    def _init_weight(self):
        # head.py:22-29 iterates this head's own modules: the encoders' attention-pool projections are not among them
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight, a=0, mode="fan_out")
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def embed(self, visual_feature, textual_feature):
        if not (visual_feature.is_cuda and textual_feature.is_cuda):
            raise RuntimeError("textreid_amd.SimpleHead runs on the HIP kernel library only (CUDA tensors); no CPU fallback")
        batch_size = visual_feature.size(0)
        v = losses.linear(visual_feature.view(batch_size, -1), self.visual_embed_layer.weight, self.visual_embed_layer.bias)
        t = losses.linear(textual_feature.view(batch_size, -1), self.textual_embed_layer.weight, self.textual_embed_layer.bias)
        return v, t

    def forward(self, visual_feature, textual_feature, captions):
        visual_embed, textual_embed = self.embed(visual_feature, textual_feature)
        if self.training:
            return None, self.loss_evaluator(visual_embed, textual_embed, captions)
        return [visual_embed, textual_embed], None


def build_simple_head(cfg, visual_size, textual_size):
    return SimpleHead(cfg, visual_size, textual_size)
