"""Plain references of the loss head and the elementwise kernels (csrc/kernels/misc.hip behind
Fn.softmax_xent / colsum / loss_total, csrc/kernels/conv_p3.hip split_planes / merge_planes behind
Fn.to_planes / from_planes): fp64 or integer-exact torch / numpy, no project code, no autograd.

    softmax_xent   target = (1 - ls) * onehot + ls / ncls (tf.losses.softmax_cross_entropy);
                   row loss = logsumexp(z) - sum_c target_c * z_c;
                   dlogits  = (exp(z - logsumexp(z)) - target) * scale
    colsum         out[n] = sum_{m < M} g[m, n], and sum |g[m, n]| (what a rounding bound scales with)
    loss_total     mean(row_loss[:B]) + half_wd * sum(l2)
    split3         hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to nearest even

Inputs of any float dtype are widened to fp64 exactly. The helpers below the references (bit
patterns, units in the last place) are shared by the CPU and the GPU test files.
"""
import numpy as np
import torch


def softmax_xent_ref(logits, labels, ncls, scale, ls):
    """(row_loss [B], dlogits [B, ncls]) in fp64 from logits[:, :ncls]."""
    z = logits[:, :ncls].detach().double().cpu()
    lab = labels.detach().cpu().long().view(-1)
    lse = torch.logsumexp(z, dim=1)
    target = torch.full_like(z, float(ls) / ncls)
    target[torch.arange(z.shape[0]), lab] += 1.0 - float(ls)
    row_loss = lse - (target * z).sum(1)
    dlogits = (torch.exp(z - lse[:, None]) - target) * float(scale)
    return row_loss, dlogits


def colsum_ref(g, M, N):
    """(sum_m g[m, n], sum_m |g[m, n]|) over m < M, n < N, both fp64 [N] (on g's device)."""
    d = g[:M, :N].detach().double()
    return d.sum(0), d.abs().sum(0)


def loss_total_ref(row_loss, B, l2, half_wd):
    """mean(row_loss[:B]) + half_wd * sum(l2) as a python float (l2 None: the mean alone)."""
    t = row_loss.detach().double().view(-1)[:B].sum() / B
    if l2 is not None:
        t = t + float(half_wd) * l2.detach().double().sum()
    return float(t)


def split3_ref(x):
    """(hi, mid, lo) bf16 CPU tensors of x's shape: three round-to-nearest-even casts."""
    x = x.detach().float().cpu()
    hi = x.to(torch.bfloat16)
    r = x - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    return hi, mid, lo


# ------------------------------------------------------------------ bit-level helpers
def bf16_rne_bits(x):
    """The bf16 bit patterns (numpy uint16) of finite fp32 values by integer arithmetic alone:
    add 0x7fff + (bit 16) to the fp32 pattern and keep the upper half (round to nearest even)."""
    u = x.detach().float().cpu().contiguous().numpy().view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bits16(t):
    """The 16-bit patterns of a bf16 / fp16 tensor as int32 (CPU)."""
    return t.detach().cpu().contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bits32(t):
    """The bit patterns of an fp32 tensor as int32 (same device)."""
    return t.detach().contiguous().view(torch.int32)


def ulp16_distance(a, b):
    """Distance in units in the last place between two finite tensors of one 16-bit float type:
    sign-magnitude patterns mapped to a monotone integer line (+0 and -0 coincide)."""
    def key(t):
        u = bits16(t)
        mag = u & 0x7FFF
        return torch.where((u & 0x8000) != 0, -mag, mag)
    return (key(a) - key(b)).abs()


def domain_bits(shape, gen, emin=27, emax=253):
    """Random fp32 bit patterns with a random sign, a biased exponent in [emin, emax] and a random
    mantissa: uniform over the binades, |x| in [2^(emin - 127), 2^(emax - 126)). The defaults are
    the plane split's exact domain 2^-100 <= |x| < 2^127."""
    n = int(np.prod(shape))
    sign = torch.randint(0, 2, (n,), generator=gen, dtype=torch.int64) << 31
    expo = torch.randint(emin, emax + 1, (n,), generator=gen, dtype=torch.int64) << 23
    mant = torch.randint(0, 1 << 23, (n,), generator=gen, dtype=torch.int64)
    u = (sign | expo | mant).numpy().astype(np.uint32)
    return torch.from_numpy(u.view(np.float32).copy()).view(*shape)
