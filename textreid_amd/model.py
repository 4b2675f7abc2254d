"""Top-level module: two backbones and an embedding head (reference ``lib/models/model.py:8-45``; state-dict
prefixes ``visual_model.``, ``textual_model.``, ``embed_model.`` are the reference's).

``EMBED_HEAD: 'moco'``: the MoCo head owns the backbones' query / key copies and runs them itself.  Any other
head takes the reference's "normal" branch: the model runs the two encoders and hands the pooled features to the
head (``embeddings.build_embed``; ``'simple'``, the baseline configs)."""
import os

import torch
from torch import nn

from . import backbones
from .caption import CaptionBatch
from .embeddings import build_embed
from .embeddings.moco_head.head import build_moco_head
from .parallel import dp_active


class Model(nn.Module):
    embed_type = "moco"

    def __init__(self, cfg, vocab_dict=None):
        super().__init__()
        head = cfg.MODEL.EMBEDDING.EMBED_HEAD
        if head != "moco" and dp_active():
            raise NotImplementedError(
                f"EMBED_HEAD={head!r} under data parallelism: the global-batch exchange (parallel.gather_embeddings) is "
                "defined for the MoCo head only - run the baseline configs on one GPU")
        self.visual_model = backbones.build_visual_model(cfg)
        self.textual_model = backbones.build_textual_model(cfg, vocab_dict=vocab_dict)
        if head == "moco":
            self.embed_model = build_moco_head(cfg, self.visual_model, self.textual_model)
        else:
            self.embed_model = build_embed(cfg, self.visual_model.out_channels, self.textual_model.out_channels)
            self.embed_type = "normal"
            self._text_stream = None

    def _side_stream(self, device):
        if os.environ.get("TRID_SERIAL", "0") == "1":  # experiment: one stream, un-overlapped kernel durations
            return torch.cuda.current_stream(device)
        if self._text_stream is None or self._text_stream.device != device:
            self._text_stream = torch.cuda.Stream(device=device)
        return self._text_stream

    def forward(self, images, captions):
        """Training: dict of losses.  Eval: (image embedding, caption embedding)."""
        if self.embed_type == "moco":
            return self.embed_model(images, captions)
        cb = CaptionBatch.from_list(captions)
        if not images.is_cuda:
            raise RuntimeError("textreid_amd.Model runs on the HIP kernel library only (CUDA tensors); no CPU fallback")
        if self.training:
            # The text encoder is a chain of tiny launch-bound kernels: it runs on a side HIP stream underneath the
            # (CU-filling) image encoder and joins before the embed layers, as the MoCo head's query lane does.
            main = torch.cuda.current_stream()
            side = self._side_stream(images.device)
            # (issue order: the image encoder - the critical path - is enqueued first; the side stream waits on an event
            # recorded before it, not on whatever the main stream holds by the time the host gets to the text encoder)
            ready = torch.cuda.Event()
            ready.record(main)
            visual_feat = self.visual_model(images)
            side.wait_event(ready)
            with torch.cuda.stream(side):
                textual_feat = self.textual_model(cb)
            main.wait_stream(side)
            textual_feat.record_stream(main)
            _, losses_embed = self.embed_model(visual_feat, textual_feat, cb)
            return dict(losses_embed)
        visual_feat = self.visual_model(images)
        textual_feat = self.textual_model(cb)
        outputs_embed, _ = self.embed_model(visual_feat, textual_feat, cb)
        return outputs_embed

    @torch.no_grad()
    def encode_images(self, images):
        """eval-mode image embeddings [N,C] (engine.inference)."""
        if self.embed_type == "moco":
            return self.embed_model.encode_images(images)
        head = self.embed_model
        return losses_linear(self.visual_model(images), head.visual_embed_layer)

    @torch.no_grad()
    def encode_captions(self, captions):
        """eval-mode caption embeddings [N,C] (engine.inference)."""
        if self.embed_type == "moco":
            return self.embed_model.encode_captions(captions)
        head = self.embed_model
        return losses_linear(self.textual_model(CaptionBatch.from_list(captions)), head.textual_embed_layer)


def losses_linear(x, layer):
    from . import losses

    return losses.linear(x.view(x.size(0), -1), layer.weight, layer.bias)


def build_model(cfg, vocab_dict=None):
    return Model(cfg, vocab_dict=vocab_dict)
