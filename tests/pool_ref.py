"""fp64 reference of the pooling family (csrc/kernels/pool.hip behind Fn.pool_forward /
pool_backward / gap_forward / gap_backward) and the case table the pool tests share. Plain loops
over the output pixels (p, q) and the window taps (r, s), vectorised over N and C only; no
torch.nn.functional pooling and no autograd, independent of ops/functional.py:

    window (p, q) covers rows p*sh - pt .. p*sh - pt + kh - 1, columns q*sw - pl .. + kw - 1;
    taps outside the map are skipped.
    max:     y = the maximum; the gradient goes to the FIRST maximal tap in row-major (r, s)
             order (strict >), position r*kw + s.
    average: y = sum / cnt, cnt = the taps inside the map (kh*kw with count_include_pad);
             dx[h, w] = sum over the windows covering (h, w) of dy / cnt.

Activations are NHWC; inputs of any float dtype are widened to fp64 exactly, tap by tap. ``at``
restricts a reference to a list of map positions (all N images and C channels of each): the
result is [N, len(at), C] instead of [N, P, Q, C], for maps too large to loop over in full.
"""
import torch


def same_pads(H, W, kh, kw, sh, sw):
    """TF 'SAME' (pt, pb, pl, pr): the smaller half before, the larger after."""
    th = max((-(-H // sh) - 1) * sh + kh - H, 0)
    tw = max((-(-W // sw) - 1) * sw + kw - W, 0)
    return (th // 2, th - th // 2, tw // 2, tw - tw // 2)


def out_hw(H, W, kh, kw, sh, sw, pads):
    pt, pb, pl, pr = pads
    return (H + pt + pb - kh) // sh + 1, (W + pl + pr - kw) // sw + 1


VALID = (0, 0, 0, 0)
# name -> (H, W, kh, kw, sh, sw, pads, is_max, incl_pad); every map has H != W. The kernel each row
# reaches (launch_pool_fwd / launch_pool_bwd) is named in tests/test_pool_exact_gpu.py.
CASES = {
    "max_k3s2_same_6x10": (6, 10, 3, 3, 2, 2, (0, 1, 0, 1), True, False),
    "max_k3s2_pad1_6x10": (6, 10, 3, 3, 2, 2, (1, 1, 1, 1), True, False),
    "max_k3s2_valid_6x10": (6, 10, 3, 3, 2, 2, VALID, True, False),
    "max_k3s2_same_7x9": (7, 9, 3, 3, 2, 2, (1, 1, 1, 1), True, False),
    "max_k3s2_valid_7x10": (7, 10, 3, 3, 2, 2, VALID, True, False),
    "max_k2s2_valid_6x10": (6, 10, 2, 2, 2, 2, VALID, True, False),
    "max_k3s1_same_5x7": (5, 7, 3, 3, 1, 1, (1, 1, 1, 1), True, False),
    "max_k5s2_same_9x11": (9, 11, 5, 5, 2, 2, (2, 2, 2, 2), True, False),
    "max_k5s1_same_6x7": (6, 7, 5, 5, 1, 1, (2, 2, 2, 2), True, False),
    "max_k3x2s1_5x7": (5, 7, 3, 2, 1, 1, (1, 1, 0, 1), True, False),
    "avg_k3s1_same_5x7": (5, 7, 3, 3, 1, 1, (1, 1, 1, 1), False, False),
    "avg_k3s1_same_inclpad_5x7": (5, 7, 3, 3, 1, 1, (1, 1, 1, 1), False, True),
    "avg_k3s1_valid_5x7": (5, 7, 3, 3, 1, 1, VALID, False, False),
    "avg_k5s3_valid_17x14": (17, 14, 5, 5, 3, 3, VALID, False, False),
    "avg_k8s1_valid_8x9": (8, 9, 8, 8, 1, 1, VALID, False, False),
    # padded windows through the generic kernels (3x3/1 has kernels of its own, VALID windows are
    # all full): the only rows where their divisor differs between windows
    "avg_k3s2_same_7x10": (7, 10, 3, 3, 2, 2, (1, 1, 0, 1), False, False),
    "avg_k3s2_same_inclpad_7x10": (7, 10, 3, 3, 2, 2, (1, 1, 0, 1), False, True),
}
assert all(same_pads(*c[:6]) == c[6] for n, c in CASES.items() if "_same_" in n)


def tie_heavy(shape, gen=None, device="cpu"):
    """round(2 * relu(randn)) / 2: post-ReLU-like plateaus (58 % zeros, the rest multiples of
    0.5), exact in every 16-bit type, so nearly every window holds ties."""
    return torch.round(2 * torch.relu(torch.randn(shape, generator=gen, device=device))) / 2


def int_grad(shape, gen=None, device="cpu"):
    """Integers in [-8, 8]: every gathered sum of up to 25 windows (+ a base) is exact in bf16."""
    return torch.randint(-8, 9, shape, generator=gen, device=device).float()


def _window(x, p, q, kh, kw, sh, sw, pads, is_max, incl_pad):
    """Window (p, q) of every image: (max, first-max position) or (mean, mean |x|), each [N, C]."""
    N, H, W, C = x.shape
    h0, w0 = p * sh - pads[0], q * sw - pads[2]
    best = torch.full((N, C), -float("inf"), dtype=torch.float64)
    arg = torch.full((N, C), 255, dtype=torch.int64)
    tot = torch.zeros(N, C, dtype=torch.float64)
    mag = torch.zeros(N, C, dtype=torch.float64)
    cnt = 0
    for r in range(kh):
        for s in range(kw):
            h, w = h0 + r, w0 + s
            if h < 0 or h >= H or w < 0 or w >= W:
                continue
            v = x[:, h, w].double()
            cnt += 1
            if is_max:
                gt = v > best  # strict: the first maximal tap wins
                best = torch.where(gt, v, best)
                arg = torch.where(gt, torch.full_like(arg, r * kw + s), arg)
            else:
                tot += v
                mag += v.abs()
    if is_max:
        return best, arg
    div = kh * kw if incl_pad else max(cnt, 1)
    return tot / div, mag / div


def pool_fwd_ref(x, kh, kw, sh, sw, pads, is_max, incl_pad=False, at=None):
    """(y, aux): aux is the window-local first-max position r*kw + s (int64) of a max pool, the
    per-window mean of |x| of an average pool. ``at``: a list of output positions (p, q)."""
    N, H, W, C = x.shape
    P, Q = out_hw(H, W, kh, kw, sh, sw, pads)
    pos = [(p, q) for p in range(P) for q in range(Q)] if at is None else list(at)
    y = torch.empty(N, len(pos), C, dtype=torch.float64)
    aux = torch.empty(N, len(pos), C, dtype=torch.int64 if is_max else torch.float64)
    for i, (p, q) in enumerate(pos):
        y[:, i], aux[:, i] = _window(x, p, q, kh, kw, sh, sw, pads, is_max, incl_pad)
    if at is None:
        return y.view(N, P, Q, C), aux.view(N, P, Q, C)
    return y, aux


def pool_bwd_ref(dy, x, kh, kw, sh, sw, pads, is_max, incl_pad=False, at=None):
    """(dx, mag): mag is the sum over the windows covering a pixel of |dy| / cnt (for a max pool
    cnt = 1 and only the windows whose first maximum the pixel is count). ``at``: a list of input
    positions (h, w). x gives the map size and, for a max pool, the values."""
    N, H, W, C = x.shape
    P, Q = out_hw(H, W, kh, kw, sh, sw, pads)
    assert tuple(dy.shape) == (N, P, Q, C)
    arg = pool_fwd_ref(x, kh, kw, sh, sw, pads, True)[1] if is_max and at is None else None
    pos = [(h, w) for h in range(H) for w in range(W)] if at is None else list(at)
    dx = torch.zeros(N, len(pos), C, dtype=torch.float64)
    mag = torch.zeros(N, len(pos), C, dtype=torch.float64)
    for i, (h, w) in enumerate(pos):
        for p in range(P):
            h0 = p * sh - pads[0]
            if h < h0 or h >= h0 + kh:
                continue
            for q in range(Q):
                w0 = q * sw - pads[2]
                if w < w0 or w >= w0 + kw:
                    continue
                d = dy[:, p, q].double()
                if is_max:
                    a = arg[:, p, q] if arg is not None else _window(x, p, q, kh, kw, sh, sw, pads, True, False)[1]
                    hit = (a == (h - h0) * kw + (w - w0)).double()
                    dx[:, i] += d * hit
                    mag[:, i] += d.abs() * hit
                else:
                    cnt = kh * kw if incl_pad else ((min(h0 + kh, H) - max(h0, 0)) * (min(w0 + kw, W) - max(w0, 0)))
                    dx[:, i] += d / cnt
                    mag[:, i] += d.abs() / cnt
    if at is None:
        return dx.view(N, H, W, C), mag.view(N, H, W, C)
    return dx, mag


def gap_fwd_ref(x):
    """Global average pool [N, H, W, C] -> ([N, C] mean, [N, C] mean |x|)."""
    N, H, W, C = x.shape
    tot = torch.zeros(N, C, dtype=torch.float64)
    mag = torch.zeros(N, C, dtype=torch.float64)
    for h in range(H):
        for w in range(W):
            v = x[:, h, w].double()
            tot += v
            mag += v.abs()
    return tot / (H * W), mag / (H * W)


def gap_bwd_ref(dy, H, W):
    """dy [N, C] -> (dx [N, H, W, C] = dy / HW at every pixel, |dy| / HW of the same shape)."""
    N, C = dy.shape
    d = dy.double() / (H * W)
    dx = torch.empty(N, H, W, C, dtype=torch.float64)
    for h in range(H):
        for w in range(W):
            dx[:, h, w] = d
    return dx, dx.abs()


def border_and_sample(H, W, n_sample, gen):
    """Every border position of an H x W map plus n_sample random ones (a sorted list)."""
    pos = {(h, w) for h in range(H) for w in (0, W - 1)} | {(h, w) for h in (0, H - 1) for w in range(W)}
    hs = torch.randint(0, H, (n_sample,), generator=gen).tolist()
    ws = torch.randint(0, W, (n_sample,), generator=gen).tolist()
    return sorted(pos | set(zip(hs, ws)))


def worst(err, bound):
    """(index tuple, err, bound) of the element whose err exceeds its bound by the most."""
    exc = (err - bound).flatten()
    i = int(exc.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
    return idx, float(err.flatten()[i]), float(torch.as_tensor(bound).expand(err.shape).flatten()[i])


def assert_exact(got, ref, what=""):
    """Elementwise equality (torch.equal), reporting the worst element."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    if torch.equal(g, r):
        return
    err = (g - r).abs()
    idx, e, _ = worst(err, torch.zeros(()))
    raise AssertionError(f"{what}: {int((err != 0).sum())} of {err.numel()} elements differ; worst at {idx}: "
                         f"got {float(g[idx])}, want {float(r[idx])}")


def assert_within(got, ref, mag, eps, what=""):
    """|got - ref| <= eps * |ref| + 2^-17 * mag elementwise (eps: 2^-8 bf16, 2^-11 fp16, 2^-23
    fp32 output rounding; 2^-17 covers an fp32 sum of up to 64 terms and the rounded 1 / cnt)."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    err = (g - r).abs()
    bound = eps * r.abs() + 2.0 ** -17 * mag.double()
    bad = err > bound
    if bool(bad.any()) or not bool(torch.isfinite(g).all()):
        idx, e, b = worst(torch.nan_to_num(err, nan=float("inf")), bound)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements out of bound; worst at {idx}: "
                             f"got {float(g[idx])}, want {float(r[idx])}, |err| {e:.3e} > bound {b:.3e}")
