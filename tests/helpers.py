"""Shared test helpers: rebuild synthetic state dicts from a golden manifest."""
import math
import os

import numpy as np
import torch

from dpmn_amd.utils import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def sd_from_manifest(man, seed):
    """manifest rows 'name|d0,d1|dtype' -> synthetic state dict (float entries only by the
    synth rule; integer/derived buffers are omitted, the oracle/HIP path recompute them)."""
    sd = {}
    for row in man:
        name, shape, dtype = str(row).split("|")
        shape = tuple(int(s) for s in shape.split(",")) if shape else ()
        if dtype.startswith("float"):
            sd[name] = torch.zeros(shape, dtype=torch.float32)
        else:
            sd[name] = torch.zeros(shape, dtype=torch.int64)
    synth.synth_fill_(sd, seed=seed)
    return sd


def checksum(sd):
    skip = ("relative_position_index", "attn_mask", "num_batches_tracked")
    return float(sum(v.double().sum().item() for k, v in sd.items()
                     if torch.is_floating_point(v) and not any(s in k for s in skip) and not k.endswith(".pe")))


def t(a):
    return torch.from_numpy(np.asarray(a))


def assert_close(a, b, atol, rtol=0.0, what=""):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    assert a.shape == b.shape, "%s shape %s vs %s" % (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bad.any(), "%s max err %.3e (tol %.1e) at %d/%d elems, ref max %.3e" % (
        what, err.max().item(), atol, int(bad.sum()), a.numel(), b.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------
# Gradient fixtures: a gradient tensor is stored in full up to 4096 elements; larger ones as a digest -- float64 norm and
# sum, 64 evenly strided samples, and one projection onto a seeded probe vector (tools/gen_golden.py gen_grads/gen_step).
def grad_digest(name, g, f64=False):
    """f64: keep the digest entries in float64 (the float64 "truth" fixtures, tools/gen_golden.py gen_f64)"""
    g = g.detach().double().reshape(-1)
    n = g.numel()
    if n <= 4096:
        return {"full": g.numpy() if f64 else g.float().numpy()}
    probe = synth.uniform("probe::" + name, (n,), -1.0, 1.0, 77).double()
    step = n // 64
    return {"norm": np.array(float(g.norm())), "sum": np.array(float(g.sum())), "samples": g[::step][:64].numpy() if f64 else g[::step][:64].float().numpy(),
            "proj": np.array(float((g * probe).sum())), "absmax": np.array(float(g.abs().max()))}


def fixture_grad_names(npz, prefix=""):
    names = []
    for k in npz.files:
        if "::" in k and k.startswith(prefix):
            n = k[len(prefix):].split("::")[0]
            if n not in names:
                names.append(n)
    return names


def grad_error_vs_fixture(npz, key, g):
    """relative error of gradient tensor g against the fixture entry `key` (= prefix + name): full tensors by relative L2;
    digests by the worst of |norm| ratio, the 64 samples (relative to the tensor's max) and the seeded projection
    (relative to norm * |probe| / sqrt(n), the scale of a projected random error)."""
    g = torch.as_tensor(g).detach().cpu().double().reshape(-1)
    if key + "::full" in npz.files:
        ref = torch.from_numpy(npz[key + "::full"]).double()
        return float((g - ref).norm() / (ref.norm() + 1e-30)), float(ref.abs().max())
    d = grad_digest(key.split("/", 1)[-1], g)
    norm, amax = float(npz[key + "::norm"]), float(npz[key + "::absmax"])
    e_norm = abs(float(d["norm"]) - norm) / (norm + 1e-30)
    e_smp = float(np.abs(d["samples"].astype(np.float64) - npz[key + "::samples"].astype(np.float64)).max()) / (amax + 1e-30)
    n = g.numel()
    e_proj = abs(float(d["proj"]) - float(npz[key + "::proj"])) / (norm * (n / 3.0) ** 0.5 / n ** 0.5 + 1e-30)
    return max(e_norm, e_smp, e_proj), amax


def check_vs_f64(test, z, named, prefix="", factor=3.0, floor=1e-5, per_tensor=10.0):
    """Adjudicated gradient check against a float64 fixture (tools/gen_golden.py gen_f64).  Per tensor t (relative error metric of
    grad_error_vs_fixture): e_ours[t] = our gradient vs the float64 result, e_ref[t] = the REFERENCE's own fp32 gradient vs it (stored
    in the fixture).  fp32 round-off is order-dependent, so single tensors scatter by several x either way (the CPU oracle -- the
    reference's arithmetic in another operation order -- has per-tensor ratios from 0.1 to 12).  Two statements are asserted:
    * per MODEL: our worst tensor and our RMS over the tensors are within `factor` of the reference's own worst / RMS (floor: models
      fp32 gets right to 1e-5 anyway);
    * per TENSOR: e_ours[t] <= per_tensor * max(e_ref[t], 0.3 * RMS_t e_ref, floor) -- no single tensor may hide inside the model
      statistics (a wrong gradient is off by O(1), i.e. 10^2 ... 10^5 x these bounds).
    Tensors whose float64 gradient is exactly zero by construction (|f64| < 1e-9: conv biases in front of a batch-statistics
    BatchNorm, quirk Q11's unused weight_list -- every such tensor of the fixtures is listed by this rule, none is merely small)
    must stay at round-off level RELATIVE to the model's largest gradient entry; any other tensor, however small, takes the relative
    checks above.  Returns (worst ratio, rms ratio)."""
    ours, ref, names, zeros = [], [], [], []
    gmax = 0.0
    for n in fixture_grad_names(z, prefix):
        err, amax = grad_error_vs_fixture(z, prefix + n, named[n])
        gmax = max(gmax, amax)
        if amax < 1e-9:
            zeros.append((n, float(torch.as_tensor(named[n]).abs().max())))
            continue
        ours.append(err); ref.append(float(z[prefix + n + "::ref32_err"])); names.append(n)
    ours, ref = np.array(ours), np.array(ref)
    if zeros:
        zworst = max(zeros, key=lambda t: t[1])
        record(test, "%slargest entry of a gradient that is exactly zero in float64 (%s), relative to the model's largest gradient entry" % (prefix, zworst[0]),
               zworst[1] / max(gmax, 1e-30), 1e-5)
        assert zworst[1] <= 1e-5 * gmax, "%s%s: %s should be zero, has |g| up to %.3e (largest gradient entry of the model %.3e)" % (test, prefix, zworst[0], zworst[1], gmax)
    iw = int(ours.argmax())
    rms_ref = float(np.sqrt((ref ** 2).mean()))
    r_worst = float(ours.max() / max(ref.max(), floor))
    r_rms = float(np.sqrt((ours ** 2).mean()) / max(rms_ref, floor))
    r_each = ours / np.maximum(np.maximum(ref, 0.3 * rms_ref), floor)
    ie = int(r_each.argmax())
    record(test, "%sworst tensor vs float64: ours %.2e (%s) / reference fp32 %.2e" % (prefix, ours.max(), names[iw], ref.max()), r_worst, factor)
    record(test, "%sRMS over %d tensors vs float64: ours %.2e / reference fp32 %.2e" % (prefix, len(names), float(np.sqrt((ours ** 2).mean())),
                                                                                     rms_ref), r_rms, factor)
    record(test, "%sworst per-tensor ratio vs float64 (%s: ours %.2e / reference fp32 %.2e)" % (prefix, names[ie], ours[ie], ref[ie]), float(r_each[ie]), per_tensor)
    assert r_worst <= factor and r_rms <= factor, "%s%s: gradients are %.1fx (worst tensor %s) / %.1fx (RMS) as far from the float64 result as the reference's own fp32 gradients (allowed %.1fx)" % (
        test, prefix, r_worst, names[iw], r_rms, factor)
    assert r_each[ie] <= per_tensor, "%s%s: tensor %s is %.1fx as far from the float64 result as the reference's own fp32 gradient of it (allowed %.1fx)" % (
        test, prefix, names[ie], float(r_each[ie]), per_tensor)
    return r_worst, r_rms


# ---------------------------------------------------------------------------------------------------------------------
# Kink-aware float64 adjudication of the CMM gradient fixture.  The CMM's LeakyReLU / ReLU inputs are BatchNorm outputs of unit
# scale; among the ~2 M of them at B = 2 a handful lie within fp32 round-off of the kink (|y| ~ 1e-7: measured 6 elements below
# 2e-6 in tests/golden/grads_cmm_cnum64_f64.npz `kink_*`).  There the DERIVATIVE an fp32 implementation uses (1 or the slope) is a
# coin flip that float64 cannot arbitrate -- the imported reference's own fp32 run flips one element of en_2_1, this library's run
# one element of en_4_1 (tools/dbg_cnum64_f64.py) -- and one flip moves every gradient upstream of it by O(1e-3 ... 1e-2): two
# correct fp32 implementations differ by more than any tolerance that would still catch a wrong kernel.  The adjudication therefore
# differentiates, in float64 (the oracle's CMM, pinned to the reference's float64 gradients to 1e-9 in the same test), the SAME
# piecewise-linear branch the implementation under test took at the ambiguous elements -- its own pre-activation signs there,
# float64's everywhere else -- exactly as the step fixture's float64 run takes the fp32 run's threshold masks.
KINK_TOL = 2e-6       # |y| below this (BatchNorm outputs have unit scale) = ambiguous in fp32


def cmm_sites(sd, x1, x2, training=True):
    """[(site, pre-activation tensor)] of every activation of the oracle CMM, in call order."""
    from oracle import cmm as ocmm
    sites = []

    def hook(site, x):
        sites.append((site, x.detach()))
        return None
    with torch.no_grad():
        ocmm.cmm_forward(sd, x1, x2, training, act_hook=hook)
    return sites


def ambiguous_kinks(sites, tol=KINK_TOL):
    """[(site, flat NCHW index, value)] of the pre-activations within `tol` of the kink."""
    out = []
    for site, x in sites:
        flat = x.reshape(-1)
        for i in torch.nonzero(flat.abs() < tol).reshape(-1).tolist():
            out.append((site, i, float(flat[i])))
    return out


def cmm_grads_f64(sd, x1, x2, cot, forced=()):
    """float64 gradients of sum(out * cot) through the oracle CMM (train-mode BatchNorm) with the activation DERIVATIVE forced at
    `forced` = [(site, flat index, positive?)]; everywhere else the float64 sign decides.  Returns {name: grad} incl. x1 / x2."""
    from oracle import cmm as ocmm
    sd = {k: (v.detach().double().requires_grad_(True) if torch.is_floating_point(v) else v) for k, v in sd.items()}
    a, b = x1.detach().double().requires_grad_(True), x2.detach().double().requires_grad_(True)
    by_site = {}
    for site, i, pos in forced:
        by_site.setdefault(site, []).append((i, bool(pos)))

    def hook(site, x):
        f = by_site.get(site)
        if not f:
            return None
        pos = (x.detach() > 0).reshape(-1).clone()
        for i, v in f:
            pos[i] = v
        return pos.reshape(x.shape)
    with torch.enable_grad():
        out = ocmm.cmm_forward(sd, a, b, True, act_hook=hook)
        (out * cot.double()).sum().backward()
    g = {"x1": a.grad, "x2": b.grad}
    g.update({k: v.grad for k, v in sd.items() if torch.is_tensor(v) and v.grad is not None})
    return g


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double().reshape(-1), torch.as_tensor(b).detach().cpu().double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def check_adjudicated(test, names, e_ours, e_ref, factor=3.0, floor=1e-5, per_tensor=10.0):
    """The two statements of check_vs_f64 on explicit per-tensor error lists (ours / the reference's own fp32, both against their
    kink-adjudicated float64 gradients)."""
    ours, ref = np.array(e_ours), np.array(e_ref)
    iw = int(ours.argmax())
    rms_ref = float(np.sqrt((ref ** 2).mean()))
    r_worst = float(ours.max() / max(ref.max(), floor))
    r_rms = float(np.sqrt((ours ** 2).mean()) / max(rms_ref, floor))
    r_each = ours / np.maximum(np.maximum(ref, 0.3 * rms_ref), floor)
    ie = int(r_each.argmax())
    record(test, "worst tensor vs kink-adjudicated float64: ours %.2e (%s) / reference fp32 %.2e" % (ours.max(), names[iw], ref.max()), r_worst, factor)
    record(test, "RMS over %d tensors vs kink-adjudicated float64: ours %.2e / reference fp32 %.2e" % (len(names), float(np.sqrt((ours ** 2).mean())), rms_ref), r_rms, factor)
    record(test, "worst per-tensor ratio (%s: ours %.2e / reference fp32 %.2e)" % (names[ie], ours[ie], ref[ie]), float(r_each[ie]), per_tensor)
    assert r_worst <= factor and r_rms <= factor, "%s: gradients are %.1fx (worst tensor %s) / %.1fx (RMS) as far from the float64 result as the reference's own fp32 gradients (allowed %.1fx)" % (
        test, r_worst, names[iw], r_rms, factor)
    assert r_each[ie] <= per_tensor, "%s: tensor %s is %.1fx as far from the float64 result as the reference's own fp32 gradient of it (allowed %.1fx)" % (
        test, names[ie], float(r_each[ie]), per_tensor)
    return r_worst, r_rms


# ---------------------------------------------------------------------------------------------------------------------
# Parity-error record: GPU tests call record(test, metric, value, tol); conftest.py dumps everything at session end to
# gpurun_out/parity_errors.json (copied to profiles/ by hand after a gpurun call), so achieved errors are data, not prints.
RECORD = []


def record(test, metric, value, tol=None):
    """Rows of the mode-2 pass of the suite ("f32 via bf16x3", conftest.py _compute_mode) carry the prefix x3: -- read from the library,
    so a test that switches the mode itself is labelled by what actually ran."""
    mode = ""
    try:
        import sys
        abi = sys.modules.get("dpmn_amd._abi")
        if abi is not None and abi.lib.dpmn_get_compute_dtype() == 2:
            mode = "x3:"
    except Exception:
        pass
    RECORD.append({"test": mode + test, "metric": metric, "value": float(value), "tol": None if tol is None else float(tol)})
    return value


def max_abs_err(a, b):
    return float((torch.as_tensor(a).float().cpu() - torch.as_tensor(b).float().cpu()).abs().max())


def l2_rel(a, b):
    a, b = torch.as_tensor(a).float().cpu().double(), torch.as_tensor(b).float().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_bicubic_tables(insz, outsz):
    """precompute_coeffs + normalize_coeffs_8bpc of Resample.c for one axis, one output index at a time in Python floats -> int32
    (outsz, 2 + ksize): per output index [xmin, n, k_0 .. k_{ksize-1}] (k_j = 0 for j >= n).  The independent restatement that
    dpmn_amd.utils.resize.pil_resample_tables (vectorised) is compared against."""
    insz, outsz = int(insz), int(outsz)
    if insz < 1 or outsz < 1:
        raise ValueError("pil_bicubic_tables: sizes must be positive, got %d -> %d" % (insz, outsz))
    scale = filterscale = float(insz) / outsz
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    tab = np.zeros((outsz, 2 + ksize), np.int32)
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insz) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        tab[xx, 0], tab[xx, 1] = xmin, xmax
        for x, w in enumerate(k):
            tab[xx, 2 + x] = int(-0.5 + w * (1 << 22)) if w < 0 else int(0.5 + w * (1 << 22))
    tab.setflags(write=False)
    return tab
