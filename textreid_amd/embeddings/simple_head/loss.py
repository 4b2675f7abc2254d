"""Loss evaluator of the simple head (reference ``simple_head/loss.py:8-48``).

Holds the identity ``projection`` (state-dict name ``loss_evaluator.projection``) and evaluates the
baseline's two training losses.  ``forward`` is the place a user changes: every entry of
``textreid_amd.losses`` takes the same arguments as its reference namesake, so swapping in
``L.cmpm_loss(visual_embed, textual_embed, labels)`` / ``L.cmpc_loss(self.projection, ...)`` is a
one-line edit.
"""
import torch
from torch import nn

from ... import losses as L
from ...caption import CaptionBatch


class LossComputation(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        emb = cfg.MODEL.EMBEDDING
        self.epsilon = emb.EPSILON
        self.scale_pos = 10.0
        self.scale_neg = 40.0
        # randn first, then xavier: draws from the global RNG in the reference's order (loss.py:15-19)
        w = torch.randn(emb.FEATURE_SIZE, cfg.MODEL.NUM_CLASSES)
        nn.init.xavier_uniform_(w, gain=1)
        self.projection = nn.Parameter(w)

    def forward(self, visual_embed, textual_embed, captions):
        labels = CaptionBatch.from_list(captions).ids.long()
        return {
            "instance_loss": L.instance_loss(self.projection, visual_embed, textual_embed, labels, epsilon=self.epsilon),
            "global_align_loss": L.global_align_loss(visual_embed, textual_embed, labels, scale_pos=self.scale_pos,
                                                     scale_neg=self.scale_neg),
        }


def make_loss_evaluator(cfg):
    return LossComputation(cfg)
