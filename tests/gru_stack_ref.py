"""fp64 restatement of the STACKED text encoder (reference lib/models/backbones/gru.py:36-43,62-63,77: nn.GRU with
num_layers > 1 and dropout between the layers) on top of oracle.text._direction, and a numpy restatement of the
Philox4x32-10 draw of csrc/dropout_seq.hip.  Test infrastructure only.

Layer l >= 1 reads [h_fwd_t, h_bwd_t] of layer l - 1 (zero at t >= length, what pad_packed_sequence produces); with keep
masks the input of layer l is that sequence * mask / (1 - p) (torch.nn.GRU's definition: dropout on the output of every
layer but the last).  Only the last layer feeds the max over time; zero pad rows up to the BATCH maximum enter it."""

import numpy as np
import torch

import oracle.text as OT


def gru_keys(num_layers):
    return ["gru.weight_%s_l%d%s" % (kind, k, sfx) for k in range(num_layers) for sfx in ("", "_reverse") for kind in ("ih", "hh")]


def state_shapes(hidden, embed, num_layers):
    out = {}
    for k in range(num_layers):
        for sfx in ("", "_reverse"):
            out["gru.weight_ih_l%d%s" % (k, sfx)] = (3 * hidden, embed if k == 0 else 2 * hidden)
            out["gru.weight_hh_l%d%s" % (k, sfx)] = (3 * hidden, hidden)
    return out


def embed_input(st, table, tokens):
    """the three input forms, as oracle.text.text_forward"""
    if table is None:
        return torch.nn.functional.embedding(tokens, st["embed.weight"], padding_idx=0)
    x = table[tokens.reshape(-1)].reshape(tokens.shape[0], tokens.shape[1], -1)
    if "embed.weight" in st:
        x = torch.nn.functional.linear(x, st["embed.weight"], st["embed.bias"])
    return x


def stack_sequences(st, x, lengths, num_layers, masks=None, p=0.0):
    """x [B, L, E] -> the list of every layer's zero-padded output sequence [B, lmax, 2H] (before dropout)."""
    lengths = lengths.view(-1)
    lmax = int(lengths.max())
    seqs = []
    for k in range(num_layers):
        of = OT._direction(x, lengths, st["gru.weight_ih_l%d" % k], st["gru.weight_hh_l%d" % k], False, lmax)
        ob = OT._direction(x, lengths, st["gru.weight_ih_l%d_reverse" % k], st["gru.weight_hh_l%d_reverse" % k], True, lmax)
        x = torch.cat([of, ob], dim=2)
        seqs.append(x)
        if masks is not None and k + 1 < num_layers:
            x = x * masks[k][:, :lmax].to(x.dtype) / (1.0 - p)
    return seqs


def stack_forward(st, table, tokens, lengths, num_layers, masks=None, p=0.0):
    """-> [B, 2H] (gru.py:62-63)"""
    return stack_sequences(st, embed_input(st, table, tokens), lengths, num_layers, masks, p)[-1].max(dim=1)[0]


# --------------------------------------------------------------------------- Philox4x32-10 (Salmon et al., SC'11)
def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] uint32 arrays (broadcastable) -> [..., 4] uint32"""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def keep_mask(n, p, seed, offset):
    """The keep bytes trid_dropout_seq_fwd_f32 draws for n elements under state (seed, offset [+ draw])."""
    groups = (n + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    ctr = np.stack([g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full(groups, offset & 0xFFFFFFFF, dtype=np.uint64),
                    np.full(groups, (offset >> 32) & 0xFFFFFFFF, dtype=np.uint64)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    words = philox4x32_10(ctr, key).reshape(-1)[:n]
    threshold = int(float(np.float32(p)) * 4294967296.0)
    return (words >= np.uint32(threshold)).astype(np.uint8)
