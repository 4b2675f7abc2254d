"""CPU restatements for the masked GalleryIndex search: the packed allow words and the masked top-k of a given similarity matrix.
Plain torch on the host, checked against brute force in test_gallery_mask_cpu.py."""

import torch


def pack_words(allow):
    """bool [n] -> int64 [ceil(n / 32)] holding the uint32 words: bit (r & 31) of word (r >> 5) = allow[r], 0 beyond n"""
    allow = torch.as_tensor(allow).reshape(-1) != 0
    n = allow.numel()
    nw = (n + 31) // 32
    bits = torch.zeros(nw * 32, dtype=torch.int64)
    bits[:n] = allow.to(torch.int64)
    weights = torch.ones(32, dtype=torch.int64) << torch.arange(32, dtype=torch.int64)
    return (bits.view(nw, 32) * weights).sum(dim=1)


def words_as_int64(words_i32):
    """the int32 view a device word buffer is held in -> the uint32 values as int64 (comparable with pack_words)"""
    return words_i32.cpu().to(torch.int64) & 0xFFFFFFFF


def masked_topk(sim, allow, k):
    """sim [Q, G] f32, allow bool [G] -> (values [Q, k], rows [Q, k] int64): the k best ALLOWED columns of every row, value descending
    then row ascending; slots beyond the allowed count are (-inf, -1)"""
    sim = sim.clone()
    allow = torch.as_tensor(allow).reshape(-1) != 0
    sim[:, ~allow] = float("-inf")
    order = torch.sort(sim, dim=1, descending=True, stable=True)
    G = sim.shape[1]
    vals = torch.full((sim.shape[0], k), float("-inf"), dtype=sim.dtype)
    rows = torch.full((sim.shape[0], k), -1, dtype=torch.int64)
    m = min(k, G)
    vals[:, :m] = order.values[:, :m]
    rows[:, :m] = order.indices[:, :m]
    rows[vals == float("-inf")] = -1
    return vals, rows
