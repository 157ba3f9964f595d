"""The conv GEMM geometry on the CPU: every launch that conv_forward / conv_dgrad / conv_wgrad /
conv_bn_inference and the FC layer make (op, geometry list, cfg, splits, and for every tensor argument
its dtype, shape and strides, unit dims dropped) against tests/golden/conv_geom_launches.json, recorded with this same
harness at the commit before the geometry records (``python tests/test_conv_geom_cpu.py --record``);
and the records' field order against the order the C++ decoders export.

The harness swaps a recording stand-in for the kernel library's op namespace, makes ``Fn.native`` true
for CPU tensors of the 16-bit and fp32 types and the split-K workspace a no-op, so nothing is launched.
The recorded lists of 28..33 entries are padded to 33 with the decoder's defaults (relu 0, stats_R 0,
splits 1, oh0 0, ow0 0) and conv_igemm's removed trailing ``w_lo=None`` is dropped; nothing else may
differ."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

from azure_hc_intel_tf_amd.nn import layers as L  # noqa: E402
from azure_hc_intel_tf_amd.nn.params import ParamStore  # noqa: E402
from azure_hc_intel_tf_amd.ops import functional as Fn  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "conv_geom_launches.json")
PKG = os.path.join(os.path.dirname(HERE), "azure_hc_intel_tf_amd")
BUILDS = [("_hcb_kernels.so", "hcb"), ("_hcb_kernels_f16.so", "hcb16")]
GEOM_OPS = ("conv_igemm", "conv_igemm_bnb", "conv_igemm_inf", "conv_p3", "conv_p3_bnb", "conv_p3_inf")
GEOM_DEFAULTS = [0, 0, 1, 0, 0]  # relu, stats_R, splits, oh0, ow0
BF16, F32 = torch.bfloat16, torch.float32
N = 2


# ------------------------------------------------------------------------------------ recording
def _desc(a):
    if isinstance(a, torch.Tensor):
        # unit dims dropped: they address nothing (a [B, C] matrix and its [B, 1, 1, C] view are one operand)
        dims = [(n, st) for n, st in zip(a.shape, a.stride()) if n != 1]
        return {"t": str(a.dtype).replace("torch.", ""), "s": [n for n, _ in dims], "st": [st for _, st in dims]}
    if isinstance(a, (list, tuple)):
        return [_desc(v) for v in a]
    assert a is None or isinstance(a, (bool, int, float)), type(a)
    return a


class Recorder:
    """Stands in for torch.ops.hcb: every op call is recorded, nothing runs."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, op):
        def call(*args):
            self.calls.append([op, [_desc(a) for a in args]])
        return call


class Harness:
    def __init__(self, setattr_):
        self.rec = Recorder()
        setattr_(Fn._ext, "ops", lambda: self.rec)
        setattr_(Fn, "native", lambda t: Fn.is_planes(t) or t.dtype in (BF16, torch.float16, F32))
        setattr_(Fn, "ensure_splitk_workspace", lambda device: None)
        # a fixed tuning table: heuristics everywhere but one fused-BN-backward and one plane entry
        setattr_(Fn, "_tuned", {Fn.dgb_key(N * 8 * 8, 64, 576, 9): [13, 2], Fn.fwd3_key(N * 8 * 8, 64, 576, 9): [7, 3]})
        setattr_(Fn, "_phase_packs", {})
        self._set = setattr_

    def det(self, on):
        self._set(Fn, "_DET", [bool(on)])

    def take(self):
        out, self.rec.calls = self.rec.calls, []
        return out


# ------------------------------------------------------------------------------------ operands
def act(shape, p3, ld_=None, off=0, dtype=None):
    """An activation [N,H,W,C]: 16-bit tensor, Planes (p3) or, ``dtype`` given, a tensor of that type;
    ``ld_``: a channel window at ``off`` of a wider buffer."""
    full = tuple(shape[:-1]) + (ld_ or shape[-1],)
    if dtype is not None:
        t = torch.zeros(full, dtype=dtype)
    elif p3:
        t = Fn.Planes.empty(full, "cpu")
        t.t.zero_()
    else:
        t = torch.zeros(full, dtype=BF16)
    return t[..., off:off + shape[-1]] if ld_ else t


def pack(n, p3):
    w = torch.zeros(n, dtype=BF16)
    Fn.register_lo(w, torch.zeros((2, n), dtype=BF16) if p3 else None)
    return w


def conv_spec(cin, cout, kh, kw, s=1, mode="SAME", d=1, H=8, W=8):
    pt, pb, pl, pr = L.resolve_pads(mode, H, W, kh, kw, s, s, d, d)
    return Fn.ConvSpec(cin=cin, cin_pad=cin, cout=cout, kh=kh, kw=kw, sh=s, sw=s, pt=pt, pl=pl, pb=pb, pr=pr, dh=d, dw=d)


def stem():
    ps = ParamStore()
    return L.StemS2D(ps, "stem", (16, 16, 8), 64, need_dx=False)


def specs():
    """({name: (spec, H, W)}, (the stem's folded spec, its input's pixel shape))."""
    st = stem()
    out = {
        "1x1": (conv_spec(32, 64, 1, 1), 8, 8),
        "3x3patch": (conv_spec(64, 64, 3, 3), 8, 8),
        "3x3s2_even": (conv_spec(16, 32, 3, 3, 2), 8, 8),
        "3x3s2_odd": (conv_spec(16, 32, 3, 3, 2, H=9, W=9), 9, 9),
        "1x1s2_even": (conv_spec(32, 64, 1, 1, 2, "VALID"), 8, 8),
        "1x1s2_odd": (conv_spec(32, 64, 1, 1, 2, "VALID", H=9, W=9), 9, 9),
        "1x7": (conv_spec(16, 24, 1, 7), 8, 9),
        "7x1": (conv_spec(16, 24, 7, 1, H=9, W=8), 9, 8),
        "3x3dil2": (conv_spec(16, 32, 3, 3, d=2), 8, 8),
        "5x5": (conv_spec(8, 16, 5, 5), 8, 8),
        "cout1001": (conv_spec(32, 1001, 1, 1), 8, 8),
    }
    return out, (st.fold_spec, st.fold_shape)


# cfg arguments per path: None, an int, (cfg, splits > 1), a retired / patch cfg
CFGS = {False: (None, 5, (13, 2), 17), True: (None, 3, (7, 2), (23, 1))}
WCFGS = {False: (None, (3, 4)), True: (None, (6, 4))}


def drive_conv(h, name, spec, H, W, p3, windows=False, raw32=False):
    """Every op of one conv on one path; ``windows``: the input a channel window, the outputs concat
    windows; ``raw32`` (plane path): fp32 tensors where Planes are converted on the way in."""
    out = {}
    P, Q = spec.out_hw(H, W)
    cin, cout = spec.cin_pad, spec.cout
    co8 = (cout + 7) // 8 * 8
    xld = cin + 16 if windows else None
    old = co8 + 24 if windows else (co8 if co8 != cout else None)
    dt32 = F32 if raw32 else None
    wp, wtr = pack(cout * spec.Kpad, p3), pack(cin * spec.Kpad_t, p3)
    x = act((N, H, W, cin), p3, xld, 8, dtype=dt32)
    vec = lambda n=cout: torch.zeros(n, dtype=F32)  # noqa: E731
    fwd = [dict(), dict(residual=True, relu=True, o32=True), dict(stats=True, stats_R=0, shift=True),
           dict(stats=True, stats_R=4, bias=True, det=True)]
    for i, (cfg, v) in enumerate(zip(CFGS[p3], fwd)):
        h.det(v.get("det", False))
        odt = F32 if (p3 or v.get("o32")) else BF16
        o = act((N, P, Q, cout), False, old, 16 if windows else 0, dtype=odt)
        res = act((N, P, Q, cout), False, old, 0, dtype=odt) if v.get("residual") else None
        stats = torch.zeros(64 * 2 * cout, dtype=F32) if v.get("stats") else None
        Fn.conv_forward(x, spec, wp, None, o, stats=stats, bias=vec() if v.get("bias") else None, cfg=cfg,
                        relu=v.get("relu", False), stats_R=v.get("stats_R", 0), residual=res,
                        stats_shift=vec() if v.get("shift") else None)
        out[f"fwd{i}"] = h.take()
    # inference: the forward plan, a patch / persistent cfg (their twins run), 16-bit / Planes / fp32 outputs
    inf = [dict(cfg=None), dict(cfg=17 if not p3 else 18, residual=True, relu=True),
           dict(cfg=(13, 2) if not p3 else (7, 2), o32=True, residual=True), dict(cfg=3, res_other=True, det=True)]
    for i, v in enumerate(inf):
        h.det(v.get("det", False))
        if p3:
            o = act((N, P, Q, cout), not v.get("o32"), old, 0, dtype=F32 if v.get("o32") else None)
        else:
            o = act((N, P, Q, cout), False, old, 0, dtype=F32 if v.get("o32") else BF16)
        res = None
        if v.get("residual"):
            res = act((N, P, Q, cout), Fn.is_planes(o), old, 0, dtype=None if Fn.is_planes(o) else o.dtype)
        elif v.get("res_other") and p3 and cout % 8 == 0 and not windows:  # a residual in the other format is converted
            res = act((N, P, Q, cout), False, None, 0, dtype=F32)
        elif v.get("res_other"):
            continue
        Fn.conv_bn_inference(x, spec, wp, None, vec(), vec(), vec(), vec(), 1e-3, o, v.get("relu", False),
                             residual=res, cfg=v["cfg"])
        out[f"inf{i}"] = h.take()
    h.det(False)
    if spec.pr < 0:  # the stem's row-window spec has no data gradient
        dgrads = []
    else:
        dgrads = [dict(cfg=None), dict(cfg=CFGS[p3][1], acc=True, dx32=True), dict(cfg=None, bnb=1),
                  dict(cfg=CFGS[p3][2], acc=True, bnb=2), dict(cfg=CFGS[p3][2], det=True, bnb=0), dict(cfg=None, acc=True)]
    dz = act((N, P, Q, cout), p3, old, 0, dtype=dt32)
    for i, v in enumerate(dgrads):
        h.det(v.get("det", False))
        dxt = F32 if (p3 or v.get("dx32")) else BF16
        dx = act((N, H, W, cin), False, xld, 0, dtype=dxt)
        bnb = None
        if "bnb" in v:
            z = act((N, H, W, cin), False, xld, 8, dtype=F32 if p3 else BF16)
            y = act((N, H, W, cin), p3, xld, 8)
            bnb = Fn.BNBwdFuse(z, y, Fn.BNSaved(vec(cin), vec(cin)), vec(cin), vec(cin), v["bnb"],
                               torch.zeros(4 * 2 * cin, dtype=F32), 4)
        Fn.conv_dgrad(dz, spec, wtr, None, dx, v.get("acc", False), cfg=v["cfg"], bnb=bnb)
        out[f"dgrad{i}"] = h.take()
    for i, (cfg, det) in enumerate([(WCFGS[p3][0], False), (WCFGS[p3][1], False), (WCFGS[p3][1], True)]):
        h.det(det)
        dw = torch.zeros((cout, spec.K), dtype=F32)
        Fn.conv_wgrad(dz, x, spec, dw, cfg=cfg)
        out[f"wgrad{i}"] = h.take()
    h.det(False)
    return {f"{name}/{k}": v for k, v in out.items()}


def drive_fc(h, p3):
    out = {}
    ps = ParamStore()
    fc = L.Logits(ps, "fc", 64, 1001)
    ps.finalize("cpu")
    fc.pack.pack, fc.pack.tr = pack(1001 * fc.pack.Kpad, p3), pack(64 * fc.pack.Kpad_t, p3)
    for det in (False, True):
        h.det(det)
        x = act((N, 64), p3)
        logits = fc.forward(x)
        out[f"fc/forward/det{int(det)}"] = h.take()
        assert logits.shape == (N, 1008)
        fc.backward(torch.zeros((N, 1008), dtype=F32 if p3 else BF16))
        out[f"fc/backward/det{int(det)}"] = h.take()
    h.det(False)
    return out


def record(setattr_):
    """case id -> the launches it made, for both paths."""
    h = Harness(setattr_)
    out = {}
    table, (fold_spec, fold_shape) = specs()
    for p3 in (False, True):
        path = "planes" if p3 else "a16"
        got = {}
        for name, (spec, H, W) in table.items():
            got.update(drive_conv(h, name, spec, H, W, p3))
        got.update(drive_conv(h, "windows", conv_spec(32, 64, 3, 3), 8, 8, p3, windows=True))
        got.update(drive_conv(h, "windows_1x1s2", conv_spec(32, 64, 1, 1, 2, "VALID"), 8, 8, p3, windows=True))
        if p3:
            got.update(drive_conv(h, "raw32", conv_spec(32, 64, 3, 3, 2), 8, 8, p3, windows=True, raw32=True))
        # the folded space-to-depth stem as StemS2D builds it: 16-channel pixels read as 64-channel row windows
        Hf, Wf, Cf = fold_shape
        x = act((N, Hf, Wf, Cf), p3)
        P, Q = fold_spec.out_hw(Hf, Wf)
        assert Fn.ld(x) < fold_spec.cin_pad
        wp = pack(64 * fold_spec.Kpad, p3)
        o = act((N, P, Q, 64), False, dtype=F32 if p3 else BF16)
        Fn.conv_forward(x, fold_spec, wp, None, o, stats=torch.zeros(4 * 2 * 64), stats_R=4, stats_shift=torch.zeros(64))
        got["stem/fwd"] = h.take()
        Fn.conv_wgrad(act((N, P, Q, 64), p3), x, fold_spec, torch.zeros((64, 256)))
        got["stem/wgrad"] = h.take()
        Fn.conv_bn_inference(x, fold_spec, wp, None, *[torch.zeros(64) for _ in range(4)], 1e-3, act((N, P, Q, 64), p3), True)
        got["stem/inf"] = h.take()
        got.update(drive_fc(h, p3))
        out.update({f"{path}/{k}": v for k, v in got.items()})
    return out


def normalise(calls):
    """A launch list as the commit before the geometry records made it -> as this one makes it."""
    out = []
    for op, args in calls:
        args = list(args)
        if op == "conv_igemm" and len(args) == 10:
            assert args[9] is None
            args = args[:9]
        if op in GEOM_OPS:
            (gi,) = [i for i, a in enumerate(args) if isinstance(a, list) and a and not isinstance(a[0], (list, dict))]
            g = args[gi]
            assert 28 <= len(g) <= 33
            args[gi] = g + GEOM_DEFAULTS[len(g) - 28:]
        out.append([op, args])
    return out


# ------------------------------------------------------------------------------------ tests
def test_launches_equal_the_recorded_ones(monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(record(monkeypatch.setattr)))
    assert sorted(got) == sorted(want)
    ops = set()
    for case in want:
        exp = normalise(want[case])
        assert got[case] == exp, f"{case}:\n got {got[case]}\nwant {exp}"
        ops.update(op for op, _ in exp)
    assert ops >= set(GEOM_OPS) | {"conv_wgrad", "conv_wgrad_p3"}
    # the sweep reached what it is there for: remap 0 / 1 / 2, phase origins, row windows, padded cout
    geoms = [a for c in got.values() for op, args in c if op in GEOM_OPS for a in args if isinstance(a, list) and len(a) == 33]
    assert {g[21] for g in geoms} == {0, 1, 2} and any(g[31] or g[32] for g in geoms)
    assert any(g[4] < g[3] for g in geoms) and any(g[17] == 1001 for g in geoms)
    assert any(g[30] > 1 for g in geoms) and any(g[29] > 0 for g in geoms)


def test_builders_take_ints_only():
    """The geometry builders are pure: ints in, records out, and always 33 / 17 entries."""
    spec = conv_spec(16, 32, 3, 3, 2)
    g = Fn.fwd_geom(spec, N, 8, 8, 16, 32)
    assert len(g) == 33 == len(Fn.ConvGeom._fields) and list(g[28:]) == GEOM_DEFAULTS
    g, (M, K, taps) = Fn.dgrad_geom(spec, N, 8, 8, 4, 4, 32, 16)
    assert len(g) == 33 and (M, K, taps) == (N * 8 * 8, 9 * 32, 9)
    assert Fn.dgrad_problem(spec, N, 8, 8, 4, 4) == (M, K)
    for phase in Fn.dgrad_phases(spec, 8, 8):
        g, prob = Fn.dgrad_phase_geom(spec, N, 8, 8, 4, 4, 32, 16, phase)
        assert len(g) == 33 and prob == Fn.dgrad_phase_problem(spec, N, phase)
    w = Fn.wgrad_geom(spec, N, 8, 8, 4, 4, 16, 32)
    assert len(w) == 17 == len(Fn.WgradGeom._fields)


@pytest.mark.parametrize("name,ns", BUILDS, ids=[ns for _, ns in BUILDS])
def test_field_order_equals_the_decoders(name, ns):
    path = os.path.join(PKG, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not built (python __graft_entry__.py builds it)")
    torch.ops.load_library(path)
    op = getattr(torch.ops, ns).conv_geom_fields
    assert tuple(op("conv")) == Fn.ConvGeom._fields
    assert tuple(op("wgrad")) == Fn.WgradGeom._fields


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], "usage: test_conv_geom_cpu.py --record [file]"
    res = record(setattr)
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        json.dump(res, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(len(res), "cases,", sum(len(v) for v in res.values()), "launches")
