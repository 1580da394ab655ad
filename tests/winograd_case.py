"""Shared pieces of tests/test_winograd.py (CPU) and tests/test_winograd_gpu.py: a torch restatement of the three stages of
include/vsx.h's vsx_conv3x3_winograd_f16 with the same rounding points (fp32 transform arithmetic; V, U, Mt and the output
rounded to fp16 once each), and the inputs both files use (SiLU-shaped activations, weights ~ N(0, 1 / K))."""
import torch
import torch.nn.functional as F

BT = torch.tensor([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]])
AT = torch.tensor([[1., 1., 1., 0.], [0., 1., -1., -1.]])
G = torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]])

REL_L2_BOUND = 2e-3          # the project's bound for a convolution (tests/test_kernels_gpu.py)
RATIO_BOUND = 3.0            # at most 3 x the direct form's error on the same inputs


def make_case(nimg, H, W, C1, C2, Cout, rowvec=False, residual=False, seed=0):
    """fp16 tensors of one convolution: x [nimg, H, W, C1] (+ x2), weight [Cout, 3, 3, C1 + C2], bias [Cout], optionally a
    row vector per image ([nimg, Cout], rows_per_vec = H * W) and a residual [nimg, H, W, Cout]."""
    g = torch.Generator().manual_seed(seed)
    C = C1 + C2
    x = F.silu(torch.randn(nimg, H, W, C, generator=g)).half()      # SiLU of a GroupNorm output: unit variance in front of it
    case = dict(x=x[..., :C1].contiguous(), x2=x[..., C1:].contiguous() if C2 else None,
                weight=(torch.randn(Cout, 3, 3, C, generator=g) / (9 * C) ** 0.5).half(),
                bias=(torch.randn(Cout, generator=g) * 0.1).half(),
                rowvec=(torch.randn(nimg, Cout, generator=g) * 0.3).half() if rowvec else None,
                residual=torch.randn(nimg, H, W, Cout, generator=g).half() if residual else None,
                rows_per_vec=H * W)
    return case


def reference(case, dtype=torch.float64):
    """F.conv2d on the fp16 values in `dtype`, then bias, row vector and residual: [nimg, H, W, Cout]"""
    x = case['x'] if case['x2'] is None else torch.cat([case['x'], case['x2']], -1)
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), case['weight'].to(dtype).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    y = y + case['bias'].to(dtype)
    if case['rowvec'] is not None:
        y = y + case['rowvec'].to(dtype)[:, None, None, :]
    if case['residual'] is not None:
        y = y + case['residual'].to(dtype)
    return y


def direct_fp16(case):
    """what the direct form can do at best: the fp64 result rounded to fp16 once"""
    return reference(case).half()


def input_transform(x):
    """x fp16 [nimg, H, W, C] -> V fp16 [16, nimg * H/2 * W/2, C]"""
    nimg, H, W, C = x.shape
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1))
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                       # [nimg, H/2, W/2, C, 4 (rows), 4 (columns)]
    v = torch.einsum('ar,nijcrs,bs->abnijc', BT, d, BT)
    return v.reshape(16, -1, C).half()


def weight_transform(weight):
    """[Cout, 3, 3, C] fp16 -> U fp16 [16, Cout, C]"""
    u = torch.einsum('ar,orsc,bs->aboc', G, weight.float(), G)
    return u.reshape(16, weight.shape[0], weight.shape[3]).half()


def output_transform(mt, nimg, H, W):
    """Mt fp16 [16, tiles, Cout] -> fp32 [nimg, H, W, Cout] (before the epilogue)"""
    m = mt.float().reshape(4, 4, nimg, H // 2, W // 2, -1)
    y = torch.einsum('pa,abnijo,qb->nipjqo', AT, m, AT)
    return y.reshape(nimg, H, W, -1)


def winograd_restated(case):
    """the three stages with the kernels' rounding points -> fp16 [nimg, H, W, Cout]"""
    x = case['x'] if case['x2'] is None else torch.cat([case['x'], case['x2']], -1)
    nimg, H, W, _ = x.shape
    v = input_transform(x)
    u = weight_transform(case['weight'])
    mt = torch.bmm(v.float(), u.float().transpose(1, 2)).half()          # fp32 sums of fp16 products, one rounding
    y = output_transform(mt, nimg, H, W)
    y = y + case['bias'].float()
    if case['rowvec'] is not None:
        y = y + case['rowvec'].float()[:, None, None, :]
    if case['residual'] is not None:
        y = y + case['residual'].float()
    return y.half()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())
