"""fp64 restatement, from the arithmetic, of the eval-mode ImageNet ResNet image encoder (reference lib/models/backbones/resnet.py:54-98,
154-167 under model.eval()) and of its pieces, on NHWC tensors.  Test infrastructure only.

conv(k, stride s, pad p):  out[b,ho,wo,n] = sum_{ky,kx,c} xp[b, s ho + ky, s wo + kx, c] w[n,ky,kx,c],  xp = x zero-padded by p,
                           Ho = (H + 2p - k) // s + 1
BatchNorm (running statistics): scale = gamma / sqrt(var + eps), shift = beta - mean * scale, y -> y * scale + shift
max pool (3, stride 2, pad 1): the maximum over the in-range taps (the padding is -inf), Hp = (H - 1) // 2 + 1
Bottleneck: out = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + identity), the stride on conv2 and on the 1x1 downsample."""

import torch

EPS = 1e-5


def conv(x, w, stride, pad):
    """x [B,H,W,C], w [N,k,k,C] (any float dtype) -> fp64 [B,Ho,Wo,N]"""
    x, w = x.double(), w.double()
    B, H, W, C = x.shape
    N, k = w.shape[0], w.shape[1]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = torch.zeros(B, H + 2 * pad, W + 2 * pad, C, dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = torch.zeros(B, Ho, Wo, N, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            tap = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out += tap @ w[:, ky, kx].t()
    return out


def ohwi(weight):
    """nn.Conv2d weight [N,C,k,k] -> [N,k,k,C]"""
    return weight.detach().cpu().permute(0, 2, 3, 1)


def bn_coeffs(gamma, beta, mean, var, eps=EPS):
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return scale, beta.double() - mean.double() * scale


def maxpool3s2(x):
    """x [B,H,W,C] -> [B,Hp,Wp,C] in x's dtype: exact (a maximum involves no arithmetic)"""
    B, H, W, C = x.shape
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((B, 2 * Hp + 1, 2 * Wp + 1, C), float("-inf"), dtype=x.dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    out = torch.full((B, Hp, Wp, C), float("-inf"), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out = torch.maximum(out, xp[:, ky:ky + 2 * (Hp - 1) + 1:2, kx:kx + 2 * (Wp - 1) + 1:2])
    return out


def conv_bn(x, conv_mod, bn_mod, relu):
    k = conv_mod.kernel_size[0]
    y = conv(x, ohwi(conv_mod.weight), conv_mod.stride[0], conv_mod.padding[0])
    scale, shift = bn_coeffs(bn_mod.weight.detach().cpu(), bn_mod.bias.detach().cpu(), bn_mod.running_mean.cpu(), bn_mod.running_var.cpu(), bn_mod.eps)
    y = y * scale + shift
    return torch.relu(y) if relu else y


def encoder(mod, images):
    """The eval-mode forward of a textreid_amd.backbones.resnet.ResNet (its parameters and buffers read as numbers; none of its
    code runs): images [B,3,H,W] -> fp64 [B,2048]."""
    x = images.detach().cpu().double().permute(0, 2, 3, 1)
    x = maxpool3s2(conv_bn(x, mod.conv1, mod.bn1, True))
    for layer in (mod.layer1, mod.layer2, mod.layer3, mod.layer4):
        for blk in layer:
            a = conv_bn(x, blk.conv1, blk.bn1, True)
            a = conv_bn(a, blk.conv2, blk.bn2, True)
            a = conv_bn(a, blk.conv3, blk.bn3, False)
            ident = x if blk.downsample is None else conv_bn(x, blk.downsample[0], blk.downsample[1], False)
            x = torch.relu(a + ident)
    return x.mean(dim=(1, 2))
