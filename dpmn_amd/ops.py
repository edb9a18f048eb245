"""Thin Python wrappers over the per-kernel C-ABI entry points (include/dpmn_hip.h).

Used by the parity tests and by host code that composes kernels outside the native module
drivers.  Every wrapper allocates its output with torch (device memory plumbing only) and
enqueues on the current HIP stream.
"""
import torch
from ._abi import stream_of as _abi_stream_of

from . import _abi
from ._abi import dptr, lib, check, stream

ACT = {"none": 0, "gelu": 1, "relu": 2, "leaky02": 3, "leaky001": 4, "mish": 5, "prelu": 6, "tanh": 7, "sigmoid": 8,
       "relu_post_res": 9}      # conv epilogue only: ReLU after the residual add


def linear(x, w, bias=None, res1=None, res2=None, act="none", slope=0.0):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device)
    check(lib.dpmn_linear_f32(dptr(x), dptr(w), dptr(bias, True), dptr(res1, True), dptr(res2, True), dptr(y), M, N, K,
                              ACT[act], float(slope), stream()))
    return y


def add_linear(x, addv, w, bias=None, act="none"):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device)
    check(lib.dpmn_add_linear_f32(dptr(x), dptr(addv), dptr(w), dptr(bias, True), dptr(y), M, N, K, ACT[act], stream()))
    return y


def cat2_linear(x1, x2, w, bias=None, act="none"):
    M, k1 = x1.shape
    k2 = x2.shape[1]
    N = w.shape[0]
    y = torch.empty(M, N, device=x1.device)
    check(lib.dpmn_cat2_linear_f32(dptr(x1), k1, dptr(x2), k2, dptr(w), dptr(bias, True), dptr(y), M, N, ACT[act], stream()))
    return y


def ln_linear(x, ln_w, ln_b, w, bias, act="none", eps=1e-5):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device)
    check(lib.dpmn_ln_linear_f32(dptr(x), dptr(ln_w), dptr(ln_b), eps, dptr(w), dptr(bias, True), dptr(y), M, N, K,
                                 ACT[act], stream()))
    return y


def patch_embed_ln(img, pe_w, pe_b, ln_w, ln_b, patch, pf_w=None, pf_b=None, p_drop=0.0, seed=0):
    """p_drop > 0: pos_drop (pgrm.py:550-551) in the kernel's epilogue, the mask of dropout(tokens, p_drop, seed)."""
    B, cin, Hi, Wi = img.shape
    Cd = pe_w.shape[0]
    tok = torch.empty(B, (Hi // patch) * (Wi // patch), Cd, device=img.device)
    check(lib.dpmn_patch_embed_ln_drop_f32(dptr(img), cin, dptr(pf_w, True), dptr(pf_b, True), dptr(pe_w), dptr(pe_b),
                                           dptr(ln_w), dptr(ln_b), dptr(tok), B, Hi, Wi, patch, Cd, float(p_drop), int(seed), stream()))
    return tok


def window_attn(q, kv, tables, windows, shifts, heads_per_group, H, W, p_drop=0.0, seed=0):
    """p_drop > 0: train-mode attn_drop (pgrm.py:248) with the mask regenerated from `seed` (include/dpmn_hip.h)."""
    B, L, Cd = q.shape
    out = torch.empty_like(q)
    check(lib.dpmn_window_attn_drop_f32(dptr(q), dptr(kv), _abi.ptr_array(tables), _abi.int_array(windows),
                                        _abi.int_array(shifts), len(windows), heads_per_group, dptr(out), B, H, W, Cd,
                                        float(p_drop), int(seed), stream()))
    return out


def ln_qkv_window_attn_supported(Cd, windows, heads_per_group, H, W):
    return bool(lib.dpmn_ln_qkv_window_attn_supported(Cd, len(windows), heads_per_group, _abi.int_array(windows), H, W))


def ln_qkv_window_attn(tq, tkv, lnq_w, lnq_b, lnkv_w, lnkv_b, wq, bq, wkv, bkv, tables, windows, shifts, heads_per_group, H, W,
                       eps=1e-5):
    """norm1_q / norm1_kv + q / kv Linear + multi-size window attention in ONE kernel (pgrm.py:322-323, 188-266); tq / tkv
    (B, L, C) are the token streams before the LayerNorms; returns the window-major `cat` tensor (B, L, C)."""
    B, L, Cd = tq.shape
    out = torch.empty_like(tq)
    ws = torch.empty(lib.dpmn_ln_qkv_window_attn_workspace_bytes() // 4, device=tq.device)      # folded weights of this call
    check(lib.dpmn_ln_qkv_window_attn_f32(dptr(tq), dptr(tkv), dptr(lnq_w), dptr(lnq_b), dptr(lnkv_w), dptr(lnkv_b), float(eps),
                                          dptr(wq), dptr(bq), dptr(wkv), dptr(bkv), _abi.ptr_array(tables), _abi.int_array(windows),
                                          _abi.int_array(shifts), len(windows), heads_per_group, dptr(out), dptr(ws), 1, B, H, W, Cd, stream()))
    return out


def ln_qkv_window_attn_d32_supported(Cd, windows, heads_per_group, H, W):
    return bool(lib.dpmn_ln_qkv_window_attn_d32_supported(Cd, len(windows), heads_per_group, _abi.int_array(windows), H, W))


def ln_qkv_window_attn_d32(tq, tkv, lnq_w, lnq_b, lnkv_w, lnkv_b, wq, bq, wkv, bkv, tables, windows, shifts, heads_per_group, H, W, eps=1e-5):
    """ln_qkv_window_attn at embed_dim 192 = 3 groups x 2 heads x 32, windows in {4, 8, 16} (csrc/attn_fused192.hip)."""
    B, L, Cd = tq.shape
    out = torch.empty_like(tq)
    ws = torch.empty(lib.dpmn_ln_qkv_window_attn_d32_workspace_bytes() // 4, device=tq.device)
    check(lib.dpmn_ln_qkv_window_attn_d32_f32(dptr(tq), dptr(tkv), dptr(lnq_w), dptr(lnq_b), dptr(lnkv_w), dptr(lnkv_b), float(eps),
                                              dptr(wq), dptr(bq), dptr(wkv), dptr(bkv), _abi.ptr_array(tables), _abi.int_array(windows),
                                              _abi.int_array(shifts), len(windows), heads_per_group, dptr(out), dptr(ws), 1, B, H, W, Cd, stream()))
    return out


def ln_qkv_window_attn_train(tq, tkv, lnq_w, lnq_b, lnkv_w, lnkv_b, wq, bq, wkv, bkv, tables, windows, shifts, heads_per_group, H, W,
                             p_drop=0.0, seed=0, eps=1e-5, save_qkv=True, fold_out=None):
    """Training forward of ln_qkv_window_attn: returns (cat, q, kv) -- q (B, L, C) and kv (B, L, 2C) are what the unfused backward
    reads; save_qkv=False: (cat, None, None) for the recomputing backward (ln_qkv_window_attn_bwd).  fold_out: a list that receives
    the folded-weight workspace of this call (the backward reuses it)."""
    B, L, Cd = tq.shape
    out = torch.empty_like(tq)
    q = torch.empty_like(tq) if save_qkv else None
    kv = torch.empty(B, L, 2 * Cd, device=tq.device) if save_qkv else None
    ws = torch.empty(lib.dpmn_ln_qkv_window_attn_workspace_bytes() // 4, device=tq.device)
    check(lib.dpmn_ln_qkv_window_attn_train_f32(dptr(tq), dptr(tkv), dptr(lnq_w), dptr(lnq_b), dptr(lnkv_w), dptr(lnkv_b), float(eps),
                                                dptr(wq), dptr(bq), dptr(wkv), dptr(bkv), _abi.ptr_array(tables), _abi.int_array(windows),
                                                _abi.int_array(shifts), len(windows), heads_per_group, dptr(out), dptr(q, True), dptr(kv, True),
                                                float(p_drop), int(seed), dptr(ws), B, H, W, Cd, stream()))
    if fold_out is not None:
        fold_out.append(ws)
    return out, q, kv


def ln_qkv_window_attn_bwd(tq, tkv, lnq_w, lnq_b, lnkv_w, lnkv_b, wq, bq, wkv, bkv, tables, windows, shifts, heads_per_group, H, W, dout,
                           p_drop=0.0, seed=0, eps=1e-5, fold=None):
    """Backward of ln_qkv_window_attn_train with q / k / v recomputed: returns (dq (B L, C), dkv (B L, 2C), [per-group partial rows of
    the bias-table gradients, (rows, table.numel())]).  fold: the forward's folded-weight workspace (None: fold again)."""
    B, L, Cd = tq.shape
    dq = torch.empty(B * L, Cd, device=tq.device)
    dkv = torch.empty(B * L, 2 * Cd, device=tq.device)
    rows = lib.dpmn_ln_qkv_window_attn_bwd_part_rows(B, H, W)
    parts = [torch.empty(rows, t.numel(), device=tq.device) for t in tables]
    ws = fold if fold is not None else torch.empty(lib.dpmn_ln_qkv_window_attn_workspace_bytes() // 4, device=tq.device)
    check(lib.dpmn_ln_qkv_window_attn_bwd_f32(dptr(tq), dptr(tkv), dptr(lnq_w), dptr(lnq_b), dptr(lnkv_w), dptr(lnkv_b), float(eps),
                                              dptr(wq), dptr(bq), dptr(wkv), dptr(bkv), _abi.ptr_array(tables), _abi.int_array(windows),
                                              _abi.int_array(shifts), len(windows), heads_per_group, dptr(dout), dptr(dq), dptr(dkv),
                                              _abi.ptr_array(parts), float(p_drop), int(seed), dptr(ws), 0 if fold is not None else 1,
                                              B, H, W, Cd, stream()))
    return dq, dkv, parts


def collate_u8(img_u8, with_mask):
    """(B, H, W, 3) uint8 (PIL-resized RGB, on the GPU) -> (B, 3 + mask, H, W) float: ToTensor + the mask channel of
    resizeNormalize (dataset.py:1266-1319)."""
    if not img_u8.is_cuda or img_u8.dtype != torch.uint8:
        raise _abi.DpmnError("collate_u8: a CUDA uint8 (B, H, W, 3) tensor is required")
    img_u8 = img_u8.contiguous()
    B, H, W, _ = img_u8.shape
    out = torch.empty(B, 4 if with_mask else 3, H, W, device=img_u8.device)
    check(lib.dpmn_collate_u8_f32(img_u8.data_ptr(), dptr(out), B, H, W, int(bool(with_mask)), stream()))
    return out


def _display_planes(x, what):
    """(tensor, pointer, batch stride, channel stride) of an NCHW fp32 CUDA tensor whose planes are contiguous."""
    if not x.is_cuda:
        raise _abi.DpmnError("display_triple: the comparison images are composed on the GPU (got a %s %s); there is no CPU "
                             "fallback" % (x.device, what))
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] < 3:
        raise _abi.DpmnError("display_triple: %s must be float32 (B, >= 3, H, W), got %s %s" % (what, x.dtype, tuple(x.shape)))
    if x.stride()[2:] != (x.shape[3], 1) or x.stride(1) < x.shape[2] * x.shape[3] or (x.shape[0] > 1 and x.stride(0) < 3 * x.stride(1)):
        x = x.contiguous()
    return x, x.data_ptr(), max(x.stride(0), 3 * x.stride(1)), x.stride(1)      # (the batch stride of a batch of one is arbitrary)


def display_triple(image_in, image_out, image_target, sel):
    """The LR / SR / HR comparison images of tripple_display / test_display (base.py:275-326) for the images `sel` (a device int32
    tensor or a list of indices) -> (n, 3 H, W, 3) uint8 on the device: rows [0, H) image_in (B, >=3, h, w) enlarged the way
    ToPILImage + PIL's bicubic resize do, rows [H, 2H) image_out, rows [2H, 3H) image_target (B, >=3, H, W) quantised the way
    save_image does; byte for byte the reference's file content.  Channels 0..2 are read in place (strides)."""
    a, pa, abs_, acs = _display_planes(image_in, "image_in")
    o, po, obs, ocs = _display_planes(image_out, "image_out")
    t, pt, tbs, tcs = _display_planes(image_target, "image_target")
    B, _, h, w = a.shape
    H, W = t.shape[2:]
    if o.shape[0] != B or t.shape[0] != B or tuple(o.shape[2:]) != (H, W):
        raise _abi.DpmnError("display_triple: image_in (B, C, h, w), image_out and image_target (B, C, H, W) expected, got %s %s %s"
                             % (tuple(a.shape), tuple(o.shape), tuple(t.shape)))
    if h > H or w > W:
        raise NotImplementedError("display_triple: the LR input is only enlarged (%d x %d -> %d x %d asked)" % (h, w, H, W))
    if not torch.is_tensor(sel):
        sel = [int(i) for i in sel]
        if any(i < 0 or i >= B for i in sel):
            raise IndexError("display_triple: sel %s outside the batch of %d" % (sel, B))
        sel = torch.tensor(sel, dtype=torch.int32).to(a.device)
    n = sel.numel()
    out = torch.empty(n, 3 * H, W, 3, dtype=torch.uint8, device=a.device)
    if n == 0:
        return out
    tabs = _resize_tables({(w, W), (h, H)}, a.device)
    tab_h, tab_v = tabs[(w, W)], tabs[(h, H)]
    check(lib.dpmn_display_triple_u8(pa, abs_, acs, po, obs, ocs, pt, tbs, tcs, _i32(sel, "display_triple"), n, tab_h.data_ptr(),
                                     tab_v.data_ptr(), tab_h.shape[1] - 2, out.data_ptr(), B, h, w, H, W, stream()))
    return out


_RESIZE_TABLES = {}
RESIZE_TABLES_MAX = 4096      # device tables kept per (insz, outsz, device); the oldest are dropped beyond this


def _resize_tables(pairs, device):
    """{(insz, outsz): the device copy of utils.resize.pil_resample_tables(insz, outsz)} for the size pairs of one call: uploaded once
    per pair and device.  Beyond RESIZE_TABLES_MAX entries the oldest ones that this call does not use are dropped, behind a device
    synchronise: a launch queued on any stream may still read them."""
    from .utils.resize import pil_resample_tables
    keys = {p: (p[0], p[1], device.type, device.index) for p in pairs}
    for (insz, outsz), key in keys.items():
        if key not in _RESIZE_TABLES:
            _RESIZE_TABLES[key] = torch.from_numpy(pil_resample_tables(insz, outsz).copy()).to(device)
    if len(_RESIZE_TABLES) > RESIZE_TABLES_MAX:
        torch.cuda.synchronize(device)
        used = set(keys.values())
        for key in [k for k in _RESIZE_TABLES if k not in used][:len(_RESIZE_TABLES) - RESIZE_TABLES_MAX]:      # (insertion order: oldest first)
            del _RESIZE_TABLES[key]
    return {p: _RESIZE_TABLES[key] for p, key in keys.items()}


def _pack(*arrays):
    """Several contiguous int64 / int32 / float32 numpy arrays in ONE zeroed int64 buffer, each at the next 8-byte boundary ->
    (buffer, the int64 word at which each array starts)."""
    import numpy as np
    if any(a.dtype not in (np.int64, np.int32, np.float32) or not a.flags.c_contiguous for a in arrays):
        raise TypeError("_pack: contiguous int64, int32 or float32 arrays expected")
    starts = np.cumsum([0] + [(a.nbytes + 7) // 8 for a in arrays])
    buf = np.zeros(int(starts[-1]), np.int64)
    for a, at in zip(arrays, starts):
        buf[at:at + (a.nbytes + 7) // 8].view(a.dtype)[:a.size] = a.reshape(-1)
    return buf, [int(at) for at in starts[:-1]]


def _upload(dev, *arrays):
    """The host arrays of one call in one upload (_pack's buffer) -> (the device tensor, then per array the device pointer of its start,
    None for an empty one).  The tensor must outlive the launches that read it: the caller keeps it until they are queued."""
    buf, starts = _pack(*arrays)
    d = torch.from_numpy(buf).to(dev)
    return (d,) + tuple(d.data_ptr() + 8 * at if a.size else None for a, at in zip(arrays, starts))


def _tile_table(hs, ws, tile_h, tile_w):
    """Every tile_h x tile_w tile of every h x w image, image after image in row-major tile order -> (tiles (n_tiles, 3) int32 [image,
    tile row, tile column], first (len + 1) int64: the tiles of image i are first[i] .. first[i + 1])."""
    import numpy as np
    th, tw = -(-hs // tile_h), -(-ws // tile_w)
    first = np.concatenate(([0], np.cumsum(th * tw))).astype(np.int64)
    tiles = np.empty((int(first[-1]), 3), np.int32)
    for i in range(len(hs)):
        t = tiles[first[i]:first[i + 1]]
        t[:, 0] = i
        t[:, 1] = np.repeat(np.arange(th[i]), tw[i])
        t[:, 2] = np.tile(np.arange(tw[i]), th[i])
    return tiles, first


def _ragged_batch(packed, meta, what):
    """The checks every op on a pack_ragged batch shares -> meta as an int64 (B, 3) numpy array of (byte offset, h, w).  packed: the device buffer, or its size in bytes where the op only writes (degrade_noise)."""
    import numpy as np
    from .utils.resize import MAX_SIDE
    if not isinstance(packed, int) and (not torch.is_tensor(packed) or not packed.is_cuda or packed.dtype != torch.uint8 or packed.dim() != 1
                                        or not packed.is_contiguous()):
        raise _abi.DpmnError("%s: a contiguous 1-D uint8 CUDA tensor is required (the uploaded pack_ragged buffer); there is no CPU "
                             "fallback" % what)
    m = np.asarray(meta.cpu() if torch.is_tensor(meta) else meta)
    if m.ndim != 2 or m.shape[1] != 3 or m.shape[0] == 0 or m.shape[0] > 65535 or m.dtype.kind not in "iu":
        raise _abi.DpmnError("%s: meta must be a non-empty integer (B, 3) array of (byte offset, h, w), B <= 65535" % what)
    m = m.astype(np.int64)
    off, hs, ws = m[:, 0], m[:, 1], m[:, 2]
    nbytes = packed if isinstance(packed, int) else packed.numel()
    if hs.min() < 1 or ws.min() < 1 or hs.max() > MAX_SIDE or ws.max() > MAX_SIDE or off.min() < 0 or int((off + hs * ws * 3).max()) > nbytes:
        raise _abi.DpmnError("%s: meta names an image outside the packed buffer or with a side outside 1 .. %d" % (what, MAX_SIDE))
    return m


def _resize_ragged_plan(packed, meta, H, W):
    """Checks and per-call device data of resize_ragged_u8 -> (B, largest h, items (B, 8) int64 on the device, workspace)."""
    import numpy as np
    from .utils.resize import MAX_SIDE
    m = _ragged_batch(packed, meta, "resize_ragged_u8")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise _abi.DpmnError("resize_ragged_u8: output size %d x %d outside 1 .. %d" % (H, W, MAX_SIDE))
    hs, ws = m[:, 1], m[:, 2]
    B, dev = m.shape[0], packed.device
    items = np.empty((B, 8), np.int64)
    items[:, :3] = m
    items[:, 3] = np.concatenate(([0], np.cumsum(hs[:-1]))) * (W * 3)      # the ragged intermediate: h x W x 3 bytes per image
    tabs = _resize_tables({(int(w), W) for w in ws} | {(int(h), H) for h in hs}, dev)
    for b in range(B):
        th, tv = tabs[(int(ws[b]), W)], tabs[(int(hs[b]), H)]
        items[b, 4:] = th.data_ptr(), th.shape[1] - 2, tv.data_ptr(), tv.shape[1] - 2
    mid = torch.empty(lib.dpmn_resize_ragged_workspace_bytes(int(hs.sum()), W), dtype=torch.uint8, device=dev)
    return B, int(hs.max()), torch.from_numpy(items).to(dev), mid


def resize_ragged_u8(packed, meta, H, W):
    """PIL's bicubic resize of a ragged batch (csrc/resize.hip): packed = the device copy of utils.resize.pack_ragged's 1-D uint8
    buffer, meta = its host (B, 3) integer array of (byte offset, h, w) -> (B, H, W, 3) uint8 on the device, byte for byte
    np.asarray(Image.fromarray(img).resize((W, H), Image.BICUBIC)) per image.  Per call one (B, 8) int64 array is uploaded; the
    coefficient tables live on the device per size pair."""
    H, W = int(H), int(W)
    B, max_h, items, mid = _resize_ragged_plan(packed, meta, H, W)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=packed.device)
    check(lib.dpmn_resize_ragged_u8(packed.data_ptr(), packed.numel(), items.data_ptr(), B, max_h, out.data_ptr(), H, W,
                                    mid.data_ptr(), mid.numel(), stream()))
    return out


DEGRADE_TILE = 32      # csrc/degrade.hip DG_TILE, csrc/psf.hip PSF_TILE


def _degrade_plan(packed, meta, what):
    """Checks and per-call host data of degrade_ragged_u8 / degrade_noise -> (meta as int64 (B, 3), items (B, 4) int64 [byte offset, h,
    w, first tile], tiles (n_tiles, 3) int32 [image, tile row, tile column]); packed: the device buffer or its size in bytes."""
    import numpy as np
    m = _ragged_batch(packed, meta, what)
    hs, ws = m[:, 1], m[:, 2]
    if int((-(-hs // DEGRADE_TILE) * -(-ws // DEGRADE_TILE)).sum()) >= 2 ** 31:      # (before the table is allocated)
        raise _abi.DpmnError("%s: the batch has more than 2^31 - 1 tiles" % what)
    tiles, first = _tile_table(hs, ws, DEGRADE_TILE, DEGRADE_TILE)
    return m, np.concatenate((m, first[:-1, None]), axis=1), tiles


def degrade_ragged_u8(packed, meta, params, z=None, seed=0):
    """Synthetic LR images of a ragged batch (csrc/degrade.hip): packed = the device copy of utils.resize.pack_ragged's buffer (the HR
    pixels), meta = its (B, 3) integer array, params = the (B, 16) rows of utils.degrade.draw_params -> the degraded images in the same
    packed layout (a new 1-D uint8 device tensor), per image utils.degrade.degrade_u8 in fp32.  z: a device float32 tensor of
    packed.numel() standard-normal values (the noise of byte i at index i), or None: generated in the kernel from `seed` (the field
    degrade_noise(seed, meta) returns).  The same arguments give the same bytes on every run."""
    import numpy as np
    m, items, tiles = _degrade_plan(packed, meta, "degrade_ragged_u8")
    B, dev = m.shape[0], packed.device
    p = np.ascontiguousarray(params.cpu().numpy() if torch.is_tensor(params) else params, dtype=np.float32)
    if p.shape != (B, 16):
        raise _abi.DpmnError("degrade_ragged_u8: params must be (%d, 16), got %s" % (B, p.shape))
    if not (np.isin(p[:, [0, 10]], (3, 5)).all() and np.isin(p[p[:, 5] == 0][:, 6], (3, 5)).all() and np.isin(p[:, 5], (0, 1)).all()
            and (p[:, [1, 11]] > 0).all() and (p[p[:, 5] == 0][:, 7] > 0).all() and (p[p[:, 5] == 1][:, 8:10] > 0).all()
            and (p[:, 3:5] >= 0).all() and np.isin(p[:, 14], (0, 1, 2)).all() and np.isfinite(p).all()):
        raise _abi.DpmnError("degrade_ragged_u8: a params row is outside its domain (kernel sizes 3 / 5, positive sigmas, "
                             "non-negative noise factors, nr_mode 0 / 1, cut_side 0 / 1 / 2)")
    if z is not None and (not torch.is_tensor(z) or not z.is_cuda or z.dtype != torch.float32 or z.dim() != 1 or not z.is_contiguous()
                          or z.numel() != packed.numel() or z.device != dev):
        raise _abi.DpmnError("degrade_ragged_u8: z must be a contiguous float32 tensor of packed.numel() values on the device of packed")
    # one upload: items, params and tiles in one int64 buffer (params / tiles reinterpreted on the device)
    n_tiles = tiles.shape[0]
    d, d_items, d_params, d_tiles = _upload(dev, items, p, tiles)
    out = torch.zeros_like(packed)      # (bytes of the buffer that belong to no image stay 0)
    ws = torch.empty(lib.dpmn_degrade_ragged_workspace_bytes(n_tiles), dtype=torch.uint8, device=dev)
    check(lib.dpmn_degrade_ragged_u8(packed.data_ptr(), packed.numel(), d_items, d_tiles, n_tiles, d_params,
                                     None if z is None else z.data_ptr(), int(seed) & (2 ** 64 - 1), B, out.data_ptr(), ws.data_ptr(),
                                     ws.numel(), stream()))
    return out


def degrade_noise(seed, meta, device=None):
    """The standard-normal field degrade_ragged_u8(..., z=None, seed=seed) uses for the images of `meta` -> float32 on the device,
    one value per packed byte ((meta[-1] offset + h * w * 3) values)."""
    import numpy as np
    if not torch.cuda.is_available():
        raise _abi.DpmnError("degrade_noise: the field is generated on the GPU; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _abi.DpmnError("degrade_noise: the field is generated on the GPU (got device %s); there is no CPU fallback" % dev)
    m = np.asarray(meta.cpu() if torch.is_tensor(meta) else meta).astype(np.int64)
    nbytes = int((m[:, 0] + m[:, 1] * m[:, 2] * 3).max()) if m.ndim == 2 and m.shape[0] and m.shape[1] == 3 else 0
    m, items, _ = _degrade_plan(nbytes, meta, "degrade_noise")
    out = torch.zeros(nbytes, dtype=torch.float32, device=dev)
    d = torch.from_numpy(items).to(dev)
    check(lib.dpmn_degrade_noise_f32(int(seed) & (2 ** 64 - 1), d.data_ptr(), nbytes, m.shape[0],
                                     int((m[:, 1] * m[:, 2]).max()), out.data_ptr(), stream()))
    return out


def _psf_tables(taps_per_image, B):
    """Checks of psf_blur_ragged_u8's PSFs -> (psf (B, 3) int32 [first tap, taps, R], taps (total, 3) int32)."""
    import numpy as np
    from .utils.psf import MAX_RADIUS, MAX_TAPS, ONE
    if torch.is_tensor(taps_per_image) or isinstance(taps_per_image, np.ndarray) or len(taps_per_image) != B:
        raise _abi.DpmnError("psf_blur_ragged_u8: taps_per_image must be a list of %d tap arrays, one per image" % B)
    arrays = [t if isinstance(t, np.ndarray) else np.asarray(t) for t in taps_per_image]
    for i, t in enumerate(arrays):
        if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu" or not (1 <= t.shape[0] <= MAX_TAPS):
            raise _abi.DpmnError("psf_blur_ragged_u8: the PSF of image %d must be an integer (n, 3) array of (dy, dx, q), 1 <= n <= %d"
                                 % (i, MAX_TAPS))
    # every other check on the concatenated list: one pass over all taps, not one per image
    flat = np.concatenate(arrays, axis=0).astype(np.int64)
    psf = np.empty((B, 3), np.int32)
    psf[:, 1] = [t.shape[0] for t in arrays]
    psf[:, 0] = np.cumsum(psf[:, 1]) - psf[:, 1]
    first = psf[:, 0].astype(np.int64)
    R = np.maximum.reduceat(np.abs(flat[:, :2]).max(axis=1), first)
    if R.max() > MAX_RADIUS:
        raise _abi.DpmnError("psf_blur_ragged_u8: the PSF of image %d has a tap with |dy| or |dx| above %d"
                             % (int(np.argmax(R > MAX_RADIUS)), MAX_RADIUS))
    bad = (np.minimum.reduceat(flat[:, 2], first) <= 0) | (np.add.reduceat(flat[:, 2], first) != ONE)
    if bad.any():
        raise _abi.DpmnError("psf_blur_ragged_u8: the PSF of image %d needs every q > 0 and sum q = %d exactly" % (int(np.argmax(bad)), ONE))
    psf[:, 2] = R
    return psf, np.ascontiguousarray(flat, dtype=np.int32)


def psf_blur_ragged_u8(packed, meta, taps_per_image):
    """A point-spread function per image of a ragged batch (csrc/psf.hip; main.py --psf_blur): packed = the device copy of
    utils.resize.pack_ragged's buffer, meta = its (B, 3) integer array, taps_per_image = B integer (n, 3) arrays of (dy, dx, q) as
    utils.psf.psf_taps / draw_psf return them (|dy|, |dx| <= 10, q > 0, sum q = 65536, at most 441 taps; the identity leaves its image
    as it is) -> the blurred images in the same packed layout (a new 1-D uint8 device tensor), per image byte for byte
    utils.psf.psf_blur_u8.  One upload and one launch per call; integer arithmetic, the same bytes on every run and in every compute
    mode."""
    m, items, tiles = _degrade_plan(packed, meta, "psf_blur_ragged_u8")
    psf, taps = _psf_tables(taps_per_image, m.shape[0])
    d, d_items, d_tiles, d_psf, d_taps = _upload(packed.device, items, tiles, psf, taps)
    out = torch.zeros_like(packed)      # (bytes of the buffer that belong to no image stay 0)
    check(lib.dpmn_psf_blur_ragged_u8(packed.data_ptr(), packed.numel(), d_items, d_tiles, tiles.shape[0], d_psf, d_taps, taps.shape[0],
                                      m.shape[0], out.data_ptr(), stream()))
    return out


def cutblur_ragged_u8(low, packed, meta, params):
    """Cutblur as a step of its own (csrc/psf.hip): low = a synthesised LR batch in the packed layout of `packed` (the HR pixels), meta =
    their (B, 3) integer array, params = (B, 16) rows of utils.degrade.draw_params, of which only cut_x and cut_side are read -> `low`
    itself, where for every image with cut_side 1 (2) the columns >= (<) cut_x now are the HR image's (utils.psf.cutblur_u8).  One upload
    and one launch; no launch at all when no image has a cut."""
    import numpy as np
    from .utils.degrade import CUT_X, CUT_SIDE
    m = _ragged_batch(packed, meta, "cutblur_ragged_u8")
    if (not torch.is_tensor(low) or low.device != packed.device or low.dtype != torch.uint8 or low.shape != packed.shape
            or not low.is_contiguous() or low.data_ptr() == packed.data_ptr()):
        raise _abi.DpmnError("cutblur_ragged_u8: low must be another contiguous uint8 tensor of packed's size on its device")
    p = np.asarray(params.cpu().numpy() if torch.is_tensor(params) else params, dtype=np.float32)
    B = m.shape[0]
    if p.shape != (B, 16):
        raise _abi.DpmnError("cutblur_ragged_u8: params must be (%d, 16), got %s" % (B, p.shape))
    cut = p[:, [CUT_X, CUT_SIDE]]
    if not (np.isfinite(cut).all() and (cut == np.floor(cut)).all() and np.isin(cut[:, 1], (0, 1, 2)).all() and (cut[:, 0] >= 0).all()
            and (cut[:, 0] <= m[:, 2]).all()):
        raise _abi.DpmnError("cutblur_ragged_u8: a params row is outside its domain (cut_side 0 / 1 / 2, cut_x an integer in 0 .. w)")
    if not cut[:, 1].any():
        return low
    cuts = np.ascontiguousarray(np.concatenate((m, cut.astype(np.int64)), axis=1))
    d, d_cuts = _upload(packed.device, cuts)
    check(lib.dpmn_cutblur_ragged_u8(packed.data_ptr(), packed.numel(), d_cuts, B, int((m[:, 1] * m[:, 2]).max()), low.data_ptr(), stream()))
    return low


RENDER_TILE = (8, 128)      # csrc/render.hip RD_TILE_H, RD_TILE_W


def render_words_u8(words_cls, lengths, params, atlases, device=None, out=None):
    """HR text crops of a batch of words (csrc/render.hip; main.py --train_words): words_cls (B, 25) integer glyph classes, lengths (B),
    params (B, 24) = what utils.render.draw_render returns, atlases = utils.render.build_atlases(...) -> (packed, meta): the images
    back to back in a 1-D uint8 device tensor and the int64 (B, 3) host tensor of (byte offset, h, w) -- the pair
    utils.resize.pack_ragged gives for the same images (utils.render.render_meta computes the sizes), byte for byte
    utils.render.render_u8 per image, ready for degrade_ragged_u8 and resize_ragged_u8.  One launch; the atlases live on the device
    per Atlases object.  out: a contiguous 1-D uint8 device tensor of at least the packed size to write into (bytes outside the images'
    extents are left alone; the first returned item is then `out` itself)."""
    import numpy as np
    from .utils import render as rd
    if not torch.cuda.is_available():
        raise _abi.DpmnError("render_words_u8: the images are rendered on the GPU; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _abi.DpmnError("render_words_u8: the images are rendered on the GPU (got device %s); there is no CPU fallback" % dev)
    to_np = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    try:
        cls, lens, p = rd.check_render(to_np(words_cls), to_np(lengths), to_np(params), atlases)
        m = rd.render_meta(cls, lens, p, atlases)
    except ValueError as e:
        raise _abi.DpmnError("render_words_u8: %s" % e)
    B = m.shape[0]
    nbytes = int(m[-1, 0] + m[-1, 1] * m[-1, 2] * 3)
    if B > 65535 or nbytes > 2 ** 31 - 1:
        raise _abi.DpmnError("render_words_u8: at most 65535 images and 2^31 - 1 bytes per batch")
    tiles, first = _tile_table(m[:, 1], m[:, 2], *RENDER_TILE)
    n_tiles = tiles.shape[0]
    # one upload: meta + first tile, params, classes, lengths and tiles in one int64 buffer (the int32 parts reinterpreted on the
    # device); the entry point also reads the host copy
    host, (o_meta, o_par, o_cls, o_len, o_til) = _pack(np.concatenate((m, first[:-1, None]), axis=1), p, cls, lens, tiles)
    d = torch.from_numpy(host).to(dev)
    key = (dev.type, dev.index)
    if key not in atlases._device:
        atlases._device[key] = (torch.from_numpy(atlases.alpha).to(dev), torch.from_numpy(atlases.advance).to(dev),
                                torch.from_numpy(atlases.height).to(dev))
    alpha, adv, hts = atlases._device[key]
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or out.device != dev or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
          or out.numel() < nbytes):
        raise _abi.DpmnError("render_words_u8: out must be a contiguous 1-D uint8 tensor of at least %d bytes on %s" % (nbytes, dev))
    dp, hp = d.data_ptr(), host.ctypes.data
    check(lib.dpmn_render_words_u8(dp + 8 * o_cls, dp + 8 * o_len, dp + 8 * o_par, alpha.data_ptr(), adv.data_ptr(),
                                   hts.data_ptr(), dp + 8 * o_meta, dp + 8 * o_til, n_tiles, out.data_ptr(), out.numel(), B,
                                   atlases.n_fonts, alpha.shape[3], alpha.shape[4], hp + 8 * o_cls, hp + 8 * o_len, hp + 8 * o_par,
                                   hp + 8 * o_meta, stream()))
    return out, torch.from_numpy(m)


def render_words_fx_u8(words_cls, lengths, params, fx, atlases, pool=None, device=None, out=None):
    """render_words_u8 with an outline, a drop shadow and a photo background per sample (csrc/render.hip k_render_words_fx; main.py
    --train_words_fx): fx (B, 20) = the rows of utils.render.draw_render_fx, pool = the utils.render.Backgrounds (None: no row may
    have the texture bit) -> (packed, meta) in the same layout and at the same sizes, byte for byte utils.render.render_fx_u8 per
    image; a row of zeros gives render_words_u8's image.  One launch; the pool is uploaded once per device and kept on the pool
    object, like the atlases.  Validated on the host; no CPU fallback."""
    import numpy as np
    from .utils import render as rd
    if not torch.cuda.is_available():
        raise _abi.DpmnError("render_words_fx_u8: the images are rendered on the GPU; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _abi.DpmnError("render_words_fx_u8: the images are rendered on the GPU (got device %s); there is no CPU fallback" % dev)
    to_np = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    try:
        cls, lens, p = rd.check_render(to_np(words_cls), to_np(lengths), to_np(params), atlases)
        m = rd.render_meta(cls, lens, p, atlases)
        fxr = rd.check_render_fx(to_np(fx), pool, n=m.shape[0])
    except ValueError as e:
        raise _abi.DpmnError("render_words_fx_u8: %s" % e)
    B = m.shape[0]
    nbytes = int(m[-1, 0] + m[-1, 1] * m[-1, 2] * 3)
    if B > 65535 or nbytes > 2 ** 31 - 1:
        raise _abi.DpmnError("render_words_fx_u8: at most 65535 images and 2^31 - 1 bytes per batch")
    tiles, first = _tile_table(m[:, 1], m[:, 2], *RENDER_TILE)
    n_tiles = tiles.shape[0]
    # one upload, as render_words_u8's, with the fx rows in it
    host, (o_meta, o_par, o_fx, o_cls, o_len, o_til) = _pack(np.concatenate((m, first[:-1, None]), axis=1), p, fxr, cls, lens, tiles)
    d = torch.from_numpy(host).to(dev)
    key = (dev.type, dev.index)
    if key not in atlases._device:
        atlases._device[key] = (torch.from_numpy(atlases.alpha).to(dev), torch.from_numpy(atlases.advance).to(dev),
                                torch.from_numpy(atlases.height).to(dev))
    alpha, adv, hts = atlases._device[key]
    pix = tab = None
    if pool is not None:
        if key not in pool._device:
            pool._device[key] = (torch.from_numpy(pool.pixels).to(dev), torch.from_numpy(pool.table).to(dev))
        pix, tab = pool._device[key]
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or out.device != dev or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
          or out.numel() < nbytes):
        raise _abi.DpmnError("render_words_fx_u8: out must be a contiguous 1-D uint8 tensor of at least %d bytes on %s" % (nbytes, dev))
    dp, hp = d.data_ptr(), host.ctypes.data
    check(lib.dpmn_render_words_fx_u8(dp + 8 * o_cls, dp + 8 * o_len, dp + 8 * o_par, dp + 8 * o_fx, alpha.data_ptr(), adv.data_ptr(),
                                      hts.data_ptr(), dp + 8 * o_meta, dp + 8 * o_til, n_tiles,
                                      None if pix is None else pix.data_ptr(), 0 if pix is None else pix.numel(),
                                      None if tab is None else tab.data_ptr(), 0 if pool is None else pool.n_photos, out.data_ptr(),
                                      out.numel(), B, atlases.n_fonts, alpha.shape[3], alpha.shape[4], hp + 8 * o_cls, hp + 8 * o_len,
                                      hp + 8 * o_par, hp + 8 * o_fx, hp + 8 * o_meta, None if pool is None else pool.table.ctypes.data,
                                      stream()))
    return out, torch.from_numpy(m)


def render_words_warp_u8(words_cls, lengths, params, fx, warp, atlases, pool=None, device=None, out=None):
    """render_words_fx_u8 with the text under a projective map and on a curved baseline per sample (csrc/render.hip
    k_render_words_warp; main.py --train_words_warp): warp (B, 16) = the rows of utils.render.draw_render_warp -> (packed, meta) in the
    same layout at the sizes of utils.render.render_warp_meta, byte for byte utils.render.render_warp_u8 per image; a warp row whose
    flags are 0 gives render_words_fx_u8's image.  One upload of the rows, one launch.  Validated on the host; no CPU fallback."""
    import numpy as np
    from .utils import render as rd
    if not torch.cuda.is_available():
        raise _abi.DpmnError("render_words_warp_u8: the images are rendered on the GPU; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _abi.DpmnError("render_words_warp_u8: the images are rendered on the GPU (got device %s); there is no CPU fallback" % dev)
    to_np = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    try:
        cls, lens, p = rd.check_render(to_np(words_cls), to_np(lengths), to_np(params), atlases)
        fxr = rd.check_render_fx(to_np(fx), pool, n=lens.shape[0])
        wr = rd.check_render_warp(to_np(warp), p, n=lens.shape[0])
        m = rd.render_warp_meta(cls, lens, p, wr, atlases)
    except ValueError as e:
        raise _abi.DpmnError("render_words_warp_u8: %s" % e)
    B = m.shape[0]
    nbytes = int(m[-1, 0] + m[-1, 1] * m[-1, 2] * 3)
    if B > 65535 or nbytes > 2 ** 31 - 1:
        raise _abi.DpmnError("render_words_warp_u8: at most 65535 images and 2^31 - 1 bytes per batch")
    tiles, first = _tile_table(m[:, 1], m[:, 2], *RENDER_TILE)
    n_tiles = tiles.shape[0]
    # one upload, as render_words_fx_u8's, with the warp rows in it
    host, (o_meta, o_par, o_fx, o_wr, o_cls, o_len, o_til) = _pack(np.concatenate((m, first[:-1, None]), axis=1), p, fxr, wr, cls, lens, tiles)
    d = torch.from_numpy(host).to(dev)
    key = (dev.type, dev.index)
    if key not in atlases._device:
        atlases._device[key] = (torch.from_numpy(atlases.alpha).to(dev), torch.from_numpy(atlases.advance).to(dev),
                                torch.from_numpy(atlases.height).to(dev))
    alpha, adv, hts = atlases._device[key]
    pix = tab = None
    if pool is not None:
        if key not in pool._device:
            pool._device[key] = (torch.from_numpy(pool.pixels).to(dev), torch.from_numpy(pool.table).to(dev))
        pix, tab = pool._device[key]
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or out.device != dev or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
          or out.numel() < nbytes):
        raise _abi.DpmnError("render_words_warp_u8: out must be a contiguous 1-D uint8 tensor of at least %d bytes on %s" % (nbytes, dev))
    dp, hp = d.data_ptr(), host.ctypes.data
    check(lib.dpmn_render_words_warp_u8(dp + 8 * o_cls, dp + 8 * o_len, dp + 8 * o_par, dp + 8 * o_fx, dp + 8 * o_wr, alpha.data_ptr(),
                                        adv.data_ptr(), hts.data_ptr(), dp + 8 * o_meta, dp + 8 * o_til, n_tiles,
                                        None if pix is None else pix.data_ptr(), 0 if pix is None else pix.numel(),
                                        None if tab is None else tab.data_ptr(), 0 if pool is None else pool.n_photos, out.data_ptr(),
                                        out.numel(), B, atlases.n_fonts, alpha.shape[3], alpha.shape[4], hp + 8 * o_cls, hp + 8 * o_len,
                                        hp + 8 * o_par, hp + 8 * o_fx, hp + 8 * o_wr, hp + 8 * o_meta,
                                        None if pool is None else pool.table.ctypes.data, stream()))
    return out, torch.from_numpy(m)


def jpeg_roundtrip_u8(images_u8, quality, out=None):
    """JPEG artefacts (csrc/jpeg.hip): images_u8 = a contiguous (B, h, w, 3) uint8 RGB batch on the device, quality = B integers (a
    sequence or a tensor), 1 .. 100 per image or 0 for "leave this image alone" -> a new (B, h, w, 3) uint8 device tensor, per image
    byte for byte utils.jpeg.jpeg_roundtrip_u8 = what PIL reads back after save(format='JPEG', quality=q).  Sides 1 .. 1024.  out:
    the tensor to write instead of a new one; `images_u8` itself runs in place.  The qualities are uploaded (B int32) per call unless
    they already are an int32 tensor on the device; nothing synchronises."""
    import numpy as np
    from .utils.jpeg import MAX_SIDE
    if not torch.is_tensor(images_u8) or not images_u8.is_cuda:
        raise _abi.DpmnError("jpeg_roundtrip_u8: the round trip runs on the GPU (got %s); there is no CPU fallback"
                             % (images_u8.device if torch.is_tensor(images_u8) else type(images_u8).__name__))
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3 or not images_u8.is_contiguous():
        raise _abi.DpmnError("jpeg_roundtrip_u8: a contiguous uint8 (B, h, w, 3) tensor is required, got %s %s"
                             % (images_u8.dtype, tuple(images_u8.shape)))
    B, h, w, _ = images_u8.shape
    if not (1 <= B <= 65535 and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise _abi.DpmnError("jpeg_roundtrip_u8: 1 <= B <= 65535 and sides 1 .. %d, got %s" % (MAX_SIDE, tuple(images_u8.shape)))
    dev = images_u8.device
    q = np.asarray(quality.cpu() if torch.is_tensor(quality) else quality)
    if q.shape != (B,) or q.dtype.kind not in "iu":
        raise _abi.DpmnError("jpeg_roundtrip_u8: quality must be %d integers, got shape %s %s" % (B, q.shape, q.dtype))
    if q.min() < 0 or q.max() > 100:
        raise _abi.DpmnError("jpeg_roundtrip_u8: a quality is outside 0 .. 100 (0: the image is left alone)")
    if torch.is_tensor(quality) and quality.device == dev and quality.dtype == torch.int32 and quality.is_contiguous():
        qd = quality
    else:
        qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(dev)
    if out is None:
        out = torch.empty_like(images_u8)
    elif (not torch.is_tensor(out) or out.device != dev or out.dtype != torch.uint8 or out.shape != images_u8.shape
          or not out.is_contiguous()):
        raise _abi.DpmnError("jpeg_roundtrip_u8: out must be a contiguous uint8 tensor of the input's shape on its device")
    ws = torch.empty(lib.dpmn_jpeg_roundtrip_workspace_bytes(B, h, w), dtype=torch.uint8, device=dev)
    check(lib.dpmn_jpeg_roundtrip_u8(images_u8.data_ptr(), out.data_ptr(), qd.data_ptr(), B, h, w, ws.data_ptr(), ws.numel(), stream()))
    return out


def quantize_sr_u8(x):
    """save_image's quantisation of channels 0..2 of x (B, >=3, H, W) float -> (B, H, W, 3) uint8 on the device = utils.display.
    quantize_sr, the bytes of an SR image file.  The channels are read in place (strides)."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _abi.DpmnError("quantize_sr_u8: the image files are quantised on the GPU (got a %s tensor); there is no CPU fallback"
                             % (x.device if torch.is_tensor(x) else type(x).__name__))
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] < 3:
        raise _abi.DpmnError("quantize_sr_u8: float32 (B, >= 3, H, W) expected, got %s %s" % (x.dtype, tuple(x.shape)))
    B, _, H, W = x.shape
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
    if out.numel() == 0:
        return out
    x, px, bs, cs = _display_planes(x, "x")
    check(lib.dpmn_quantize_sr_u8(px, bs, cs, out.data_ptr(), B, H, W, stream()))
    return out


def _resize_windows_plan(packed, meta, lr_h, lr_w):
    """Checks and per-call host data of resize_windows_u8 -> (plan, host): plan = utils.tile's list of (image, x0) per window, host = the
    arrays of one call as numpy: items (B, 10) int64, windows (T, 2) int32, tables (1-D int32: the coefficient tables of the call's
    size pairs, each once) and the sums that size the workspace and the launches (_resize_windows_run)."""
    import numpy as np
    from .utils.resize import MAX_SIDE, pil_resample_tables
    from .utils.tile import line_width, window_plan
    m = _ragged_batch(packed, meta, "resize_windows_u8")
    if not (1 <= lr_h <= MAX_SIDE and 2 <= lr_w <= MAX_SIDE):
        raise _abi.DpmnError("resize_windows_u8: window size %d x %d outside 1 .. %d" % (lr_h, lr_w, MAX_SIDE))
    hs, ws = m[:, 1], m[:, 2]
    try:
        wl = np.array([line_width(int(h), int(w), lr_h, lr_w) for h, w in zip(hs, ws)], np.int64)
    except ValueError as e:
        raise _abi.DpmnError("resize_windows_u8: %s" % e) from e
    B = m.shape[0]
    plan = [(b, x0) for b in range(B) for x0 in window_plan(int(wl[b]), lr_w)]
    # the tables travel with the call (one upload): line widths make far more distinct size pairs than the device cache of
    # resize_ragged_u8 is sized for, and a batch reads each of its tables once
    tabs, chunks, n_ints = {}, [], 0
    for pair in [(int(w), int(l)) for w, l in zip(ws, wl)] + [(int(h), lr_h) for h in hs]:
        if pair not in tabs:
            t = pil_resample_tables(*pair)
            tabs[pair] = (n_ints, t.shape[1] - 2)
            chunks.append(t.reshape(-1))
            n_ints += t.size
    items = np.empty((B, 10), np.int64)
    items[:, :3] = m
    items[:, 3] = wl
    mid = hs * wl * 3
    items[:, 4] = np.concatenate(([0], np.cumsum(mid[:-1])))                                   # the ragged intermediate: h x w_line x 3
    items[:, 5] = int(mid.sum()) + np.concatenate(([0], np.cumsum(wl[:-1]))) * (lr_h * 3)      # behind it the lines: lr_h x w_line x 3
    for b in range(B):
        items[b, 6:8] = tabs[(int(ws[b]), int(wl[b]))]
        items[b, 8:10] = tabs[(int(hs[b]), lr_h)]
    host = dict(items=items, windows=np.asarray(plan, np.int32).reshape(-1, 2), tables=np.concatenate(chunks), lr_size=(lr_h, lr_w),
                sum_h_w_line=int((hs * wl).sum()), sum_w_line=int(wl.sum()), max_mid_bytes=int(mid.max()), max_w_line=int(wl.max()))
    return plan, host


def _resize_windows_run(packed, host):
    """One upload of the host arrays of _resize_windows_plan (items, windows and tables in one int64 buffer) and the three launches."""
    items, windows, tables, (lr_h, lr_w) = host["items"], host["windows"], host["tables"], host["lr_size"]
    B, T, dev = items.shape[0], windows.shape[0], packed.device
    d, d_items, d_windows, d_tables = _upload(dev, items, windows, tables)
    ws = torch.empty(lib.dpmn_resize_windows_workspace_bytes(host["sum_h_w_line"], host["sum_w_line"], lr_h), dtype=torch.uint8, device=dev)
    out = torch.empty(T, lr_h, lr_w, 3, dtype=torch.uint8, device=dev)
    check(lib.dpmn_resize_windows_u8(packed.data_ptr(), packed.numel(), d_items, B, d_tables, tables.size,
                                     d_windows, T, host["max_mid_bytes"], host["max_w_line"], out.data_ptr(), lr_h, lr_w,
                                     ws.data_ptr(), ws.numel(), stream()))
    return out


def resize_windows_u8(packed, meta, lr_h, lr_w):
    """A ragged batch of images as overlapping windows of the model's LR size (csrc/tile.hip): packed / meta as resize_ragged_u8 takes
    them -> (windows (T, lr_h, lr_w, 3) uint8 on the device, plan).  Every image is resized to the height lr_h and its own width
    (utils.tile.line_width; byte for byte Image.resize((w_line, lr_h), BICUBIC)) once and cut at utils.tile.window_plan's starts; plan is
    the list of (image, x0) per window that stitch_windows_u8 takes.  = utils.tile.resize_windows_np.  Per call one buffer is uploaded:
    the items, the windows and the coefficient tables of the call's size pairs."""
    plan, host = _resize_windows_plan(packed, meta, int(lr_h), int(lr_w))
    return _resize_windows_run(packed, host), plan


def stitch_windows_u8(sr, plan, scale=2):
    """The SR windows of resize_windows_u8's plan back into one image per input (csrc/tile.hip): sr (T, >= 3, H, scale * lr_w) float32
    on the device, channels 0..2 read in place -> (packed, meta): a 1-D uint8 device tensor holding the SR lines back to back (HWC) and
    the host int64 (B, 3) array of (byte offset, H, scale * w_line) per image, the layout of utils.resize.pack_ragged.  Every window is
    quantised with save_image's rule and overlapping windows are blended in integers = utils.tile.stitch_np, byte for byte."""
    import numpy as np
    from .utils.tile import plan_lines
    if not torch.is_tensor(sr) or not sr.is_cuda:
        raise _abi.DpmnError("stitch_windows_u8: the windows are stitched on the GPU (got a %s tensor); there is no CPU fallback"
                             % (sr.device if torch.is_tensor(sr) else type(sr).__name__))
    scale = int(scale)
    if sr.dtype != torch.float32 or sr.dim() != 4 or sr.shape[1] < 3 or sr.shape[0] != len(plan) or sr.shape[0] == 0 or scale < 1 or \
            sr.shape[3] % scale or sr.shape[3] < 2 * scale:
        raise _abi.DpmnError("stitch_windows_u8: float32 (T, >= 3, H, scale * lr_w) windows and a plan of T entries expected, got %s %s "
                             "and %d" % (sr.dtype, tuple(sr.shape), len(plan)))
    T, _, H, sr_w = sr.shape
    try:
        lines = plan_lines(plan, sr_w // scale)
    except ValueError as e:
        raise _abi.DpmnError("stitch_windows_u8: %s" % e) from e
    B = len(lines)
    if B > 65535:
        raise _abi.DpmnError("stitch_windows_u8: more than 65535 images")
    meta = np.empty((B, 3), np.int64)
    meta[:, 1], meta[:, 2] = H, [scale * l[2] for l in lines]
    sizes = meta[:, 1] * meta[:, 2] * 3
    meta[:, 0] = np.concatenate(([0], np.cumsum(sizes[:-1])))
    d, d_lines, d_windows = _upload(sr.device, np.array([(off, l[2], l[0], l[1]) for off, l in zip(meta[:, 0], lines)], np.int64),
                                    np.asarray(plan, np.int32).reshape(-1, 2))
    out = torch.zeros(int(sizes.sum()), dtype=torch.uint8, device=sr.device)
    x, px, bs, cs = _display_planes(sr, "sr")
    check(lib.dpmn_stitch_windows_u8(px, bs, cs, T, H, sr_w, scale, d_lines, B, d_windows, max(l[2] for l in lines),
                                     out.data_ptr(), out.numel(), stream()))
    return out, meta


QUAD_TILE = (8, 32)      # csrc/quad.hip QUAD_TILE_H, QUAD_TILE_W


def _region_tiles(hs, ws):
    """The tile table of quad_crop_u8 and poly_crop_u8: int32 (n_tiles, 3) [region, tile row, tile column], every QUAD_TILE tile of every
    h x w region, region after region in row-major tile order."""
    return _tile_table(hs, ws, *QUAD_TILE)[0]


def _quad_crop_plan(packed, meta, regions):
    """Checks and per-call host data of quad_crop_u8 -> host: the arrays of one call as numpy -- table (R, 14) int64 [byte offset of the
    photo, H, W, byte offset of the region in the output, h, w, the bits of the 8 float64 coefficients], tiles (n_tiles, 3) int32
    [region, tile row, tile column], meta (R, 3) int64 (byte offset, h, w) of the output, and its size in bytes (_quad_crop_run)."""
    import numpy as np
    from .utils.resize import MAX_PACKED_BYTES, MAX_SIDE
    m = _ragged_batch(packed, meta, "quad_crop_u8")
    R = len(regions)
    table = np.empty((R, 14), np.int64)
    for r, reg in enumerate(regions):
        try:
            b, h, w, coeffs = reg
            b, h, w = int(b), int(h), int(w)
            a = np.asarray(coeffs, np.float64).reshape(-1)
        except (TypeError, ValueError) as e:
            raise _abi.DpmnError("quad_crop_u8: region %d is not (photo index, h, w, 8 coefficients): %s" % (r, e)) from e
        if not (0 <= b < m.shape[0] and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and a.size == 8 and np.isfinite(a).all()):
            raise _abi.DpmnError("quad_crop_u8: region %d names a photo outside the batch of %d, a side outside 1 .. %d or does not "
                                 "carry 8 finite coefficients" % (r, m.shape[0], MAX_SIDE))
        table[r, :3] = m[b]
        table[r, 4:6] = h, w
        table[r, 6:] = a.view(np.int64)
    sizes = table[:, 4] * table[:, 5] * 3
    first = np.concatenate(([0], np.cumsum(sizes)))
    if first[-1] > MAX_PACKED_BYTES:
        raise _abi.DpmnError("quad_crop_u8: the regions hold more than 2^31 - 1 bytes")
    table[:, 3] = first[:-1]
    return dict(table=table, tiles=_region_tiles(table[:, 4], table[:, 5]), meta=np.ascontiguousarray(table[:, 3:6]), out_bytes=int(first[-1]))


def _quad_crop_run(packed, host, out=None):
    """One upload of the host arrays of _quad_crop_plan (the region table and the tiles in one int64 buffer) and the launch ->
    (the packed regions, the library's return code): the output exists whatever the code says.  out: a zeroed buffer of
    host["out_bytes"] bytes that the regions are written into (crop_regions_u8: shared with poly_crop_u8's regions)."""
    import numpy as np
    table, tiles = np.ascontiguousarray(host["table"], dtype=np.int64), np.ascontiguousarray(host["tiles"], dtype=np.int32)
    R, n_tiles, dev = table.shape[0], tiles.shape[0], packed.device
    if out is None:
        out = torch.zeros(host["out_bytes"], dtype=torch.uint8, device=dev)
    if R == 0:
        return out, lib.dpmn_quad_crop_u8(packed.data_ptr(), packed.numel(), None, None, 0, None, 0, None, 0, stream())
    d, d_table, d_tiles = _upload(dev, table, tiles)
    return out, lib.dpmn_quad_crop_u8(packed.data_ptr(), packed.numel(), d_table, table.ctypes.data, R, d_tiles, n_tiles,
                                      out.data_ptr(), out.numel(), stream())


def quad_crop_u8(packed, meta, regions):
    """The text regions of a ragged batch of photos, rectified (csrc/quad.hip): packed / meta as resize_ragged_u8 takes them (the
    uploaded utils.resize.pack_ragged buffer of the photos and its (B, 3) array), regions = a list of (photo index, h, w, coeffs), coeffs
    the 8 float64 coefficients of utils.quad.quad_coeffs -> (packed_regions, region_meta): a 1-D uint8 device tensor holding the R
    regions back to back as (h, w, 3) and the host int64 (R, 3) array of (byte offset, h, w) per region -- the layout of pack_ragged,
    what resize_ragged_u8 and resize_windows_u8 take.  Per region byte for byte np.asarray(Image.fromarray(photo).transform((w, h),
    Image.PERSPECTIVE, coeffs, Image.BICUBIC)) = utils.quad.quad_crop_np, in float64.  A region may reach outside its photo (black
    there).  An empty list gives empty outputs and launches nothing.  Per call one buffer is uploaded: the region table and the tiles."""
    host = _quad_crop_plan(packed, meta, list(regions))
    out, code = _quad_crop_run(packed, host)
    check(code)
    return out, host["meta"]


POLY_MAX_CELLS = 31      # csrc/poly.hip POLY_MAX_CELLS = utils.poly.MAX_POLY_SIDE - 1; its tiles are QUAD_TILE's


def _poly_crop_plan(packed, meta, regions):
    """Checks and per-call host data of poly_crop_u8 -> host: the arrays of one call as numpy -- table (R, 8) int64 [byte offset of the
    photo, H, W, byte offset of the region in the output, h, w, first cell, cell count], cells (C, 10) int64 [x0, x1, the bits of the 8
    float64 coefficients], tiles (n_tiles, 3) int32 [region, tile row, tile column], meta (R, 3) int64 (byte offset, h, w) of the
    output, and its size in bytes (_poly_crop_run)."""
    import numpy as np
    from .utils.poly import check_cells
    from .utils.resize import MAX_PACKED_BYTES, MAX_SIDE
    m = _ragged_batch(packed, meta, "poly_crop_u8")
    R = len(regions)
    table, cells = np.empty((R, 8), np.int64), []
    for r, reg in enumerate(regions):
        try:
            b, h, w, reg_cells = reg
            b, h, w = int(b), int(h), int(w)
            if not (0 <= b < m.shape[0] and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
                raise ValueError("it names a photo outside the batch of %d or a side outside 1 .. %d" % (m.shape[0], MAX_SIDE))
            bounds, coeffs = check_cells(h, w, reg_cells)
            if not np.isfinite(coeffs).all():
                raise ValueError("a coefficient is not finite")
        except (TypeError, ValueError) as e:
            raise _abi.DpmnError("poly_crop_u8: region %d is not (photo index, h, w, cells (x0, x1, 8 coefficients)): %s" % (r, e)) from e
        table[r, :3] = m[b]
        table[r, 4:] = h, w, sum(c.shape[0] for c in cells), bounds.shape[0]
        cells.append(np.concatenate([bounds, coeffs.view(np.int64)], axis=1))
    sizes = table[:, 4] * table[:, 5] * 3
    first = np.concatenate(([0], np.cumsum(sizes)))
    if first[-1] > MAX_PACKED_BYTES:
        raise _abi.DpmnError("poly_crop_u8: the regions hold more than 2^31 - 1 bytes")
    table[:, 3] = first[:-1]
    return dict(table=table, cells=np.concatenate(cells) if cells else np.empty((0, 10), np.int64), tiles=_region_tiles(table[:, 4], table[:, 5]),
                meta=np.ascontiguousarray(table[:, 3:6]), out_bytes=int(first[-1]))


def _poly_crop_run(packed, host, out=None):
    """One upload of the host arrays of _poly_crop_plan (the region table, the cells and the tiles in one int64 buffer) and the launch
    -> (the packed regions, the library's return code): the output exists whatever the code says.  out: as _quad_crop_run takes it."""
    import numpy as np
    table, cells, tiles = (np.ascontiguousarray(host[k], dtype=t) for k, t in (("table", np.int64), ("cells", np.int64), ("tiles", np.int32)))
    R, C, n_tiles, dev = table.shape[0], cells.shape[0], tiles.shape[0], packed.device
    if out is None:
        out = torch.zeros(host["out_bytes"], dtype=torch.uint8, device=dev)
    if R == 0:
        return out, lib.dpmn_poly_crop_u8(packed.data_ptr(), packed.numel(), None, None, 0, None, None, 0, None, 0, None, 0, stream())
    d, d_table, d_cells, d_tiles = _upload(dev, table, cells, tiles)
    return out, lib.dpmn_poly_crop_u8(packed.data_ptr(), packed.numel(), d_table, table.ctypes.data, R, d_cells,
                                      cells.ctypes.data, C, d_tiles, n_tiles, out.data_ptr(), out.numel(), stream())


def poly_crop_u8(packed, meta, regions):
    """Curved text regions of a ragged batch of photos, rectified (csrc/poly.hip): packed / meta as resize_ragged_u8 takes them,
    regions = a list of (photo index, h, w, cells), cells the list of (x0, x1, 8 float64 coefficients) of utils.poly.polygon_cells -- at
    most POLY_MAX_CELLS, their bounds ascending from 0 to w without a gap -> (packed_regions, region_meta) in quad_crop_u8's layout, what
    resize_ragged_u8 and resize_windows_u8 take.  Per region byte for byte np.asarray(Image.fromarray(photo).transform((w, h),
    Image.MESH, cells, Image.BICUBIC)) = utils.poly.poly_crop_np, in float64.  A region may reach outside its photo (black there).  An
    empty list gives empty outputs and launches nothing.  Per call one buffer is uploaded: the region table, the cells and the tiles."""
    host = _poly_crop_plan(packed, meta, list(regions))
    out, code = _poly_crop_run(packed, host)
    check(code)
    return out, host["meta"]


def _has_cells(region):
    """Whether a region's 4th item is poly_crop_u8's list of cells (x0, x1, coefficients) and not quad_crop_u8's 8 coefficients."""
    g = region[3] if isinstance(region, (tuple, list)) and len(region) == 4 else None
    return isinstance(g, (tuple, list)) and len(g) > 0 and isinstance(g[0], (tuple, list))


def crop_regions_u8(packed, meta, regions):
    """quad_crop_u8 and poly_crop_u8 over one list (dataset/folder.py with polygons=True): a region whose 4th item is a list of cells is
    rectified as a polygon, any other as a quadrilateral, and the regions lie in list order in ONE packed buffer -> (packed_regions,
    region_meta) as either op returns them.  Each kernel is launched once over its own regions with the byte offsets of the shared
    buffer in its table: no region is copied.  A list without polygons is quad_crop_u8 (and one without quadrilaterals poly_crop_u8)."""
    import numpy as np
    from .utils.resize import MAX_PACKED_BYTES
    regions = list(regions)
    poly = [_has_cells(r) for r in regions]
    if not any(poly):
        return quad_crop_u8(packed, meta, regions)
    if all(poly):
        return poly_crop_u8(packed, meta, regions)
    hosts = [plan(packed, meta, [r for r, p in zip(regions, poly) if p == want])
             for plan, want in ((_quad_crop_plan, False), (_poly_crop_plan, True))]
    out_meta = np.empty((len(regions), 3), np.int64)
    for host, want in zip(hosts, (False, True)):
        out_meta[[i for i, p in enumerate(poly) if p == want], 1:] = host["meta"][:, 1:]
    sizes = out_meta[:, 1] * out_meta[:, 2] * 3
    out_meta[:, 0] = np.concatenate(([0], np.cumsum(sizes[:-1])))
    total = int(sizes.sum())
    if total > MAX_PACKED_BYTES:
        raise _abi.DpmnError("crop_regions_u8: the regions hold more than 2^31 - 1 bytes")
    out = torch.zeros(total, dtype=torch.uint8, device=packed.device)
    for host, want, run in zip(hosts, (False, True), (_quad_crop_run, _poly_crop_run)):
        host["table"][:, 3] = out_meta[[i for i, p in enumerate(poly) if p == want], 0]
        host["out_bytes"] = total
        check(run(packed, host, out)[1])
    return out, out_meta


PASTE_TILE = (8, 32)      # csrc/paste_poly.hip PASTE_TILE_H, PASTE_TILE_W
PASTE_MAX_TILES = 2 ** 31 - 1      # one block per tile in the grid's x dimension


def _paste_inputs(photo2, sr_packed, sr_meta, what):
    """The checks that the paste ops share -> (H2, W2, the SR images' int64 (B, 3) meta): a contiguous (H2, W2, 3) uint8 photo on the
    device, the SR images in pack_ragged's layout on the same device, and no storage shared between the two."""
    from .utils.resize import MAX_SIDE
    if not torch.is_tensor(photo2) or not photo2.is_cuda:
        raise _abi.DpmnError("%s: the regions are pasted on the GPU (got a %s photo); there is no CPU fallback"
                             % (what, photo2.device if torch.is_tensor(photo2) else type(photo2).__name__))
    if photo2.dtype != torch.uint8 or photo2.dim() != 3 or photo2.shape[2] != 3 or not photo2.is_contiguous():
        raise _abi.DpmnError("%s: a contiguous (H2, W2, 3) uint8 photo expected, got %s %s" % (what, photo2.dtype, tuple(photo2.shape)))
    H2, W2 = int(photo2.shape[0]), int(photo2.shape[1])
    if not (1 <= H2 <= MAX_SIDE and 1 <= W2 <= MAX_SIDE):
        raise _abi.DpmnError("%s: the photo is %d x %d, sides outside 1 .. %d" % (what, H2, W2, MAX_SIDE))
    m = _ragged_batch(sr_packed, sr_meta, what)
    if sr_packed.device != photo2.device:
        raise _abi.DpmnError("%s: the photo is on %s, the SR images on %s" % (what, photo2.device, sr_packed.device))
    lo, hi = photo2.data_ptr(), photo2.data_ptr() + photo2.numel()
    if sr_packed.data_ptr() < hi and lo < sr_packed.data_ptr() + sr_packed.numel():
        raise _abi.DpmnError("%s: the photo and the SR buffer share storage (the photo is written while the SR images are read)" % what)
    return H2, W2, m


def _box_tile_ids(box, W2):
    """The row-major numbers of the PASTE_TILE tiles that a box (x0, y0, x1, y1) of the photo meets (none for an empty box)."""
    import numpy as np
    x0, y0, x1, y1 = box
    if x1 <= x0 or y1 <= y0:
        return np.empty(0, np.int64)
    th, tw = PASTE_TILE
    rows, cols = np.arange(y0 // th, (y1 - 1) // th + 1, dtype=np.int64), np.arange(x0 // tw, (x1 - 1) // tw + 1, dtype=np.int64)
    return (rows[:, None] * -(-W2 // tw) + cols[None, :]).reshape(-1)


def _paste_tiles(ids, W2, what):
    """ids: per region the numbers of the tiles it meets -> (tiles (n_tiles, 4) int32 [tile row, tile column, first, count] in
    row-major tile order, list (n_list) int32: per tile its regions in the order of the regions)."""
    import numpy as np
    owners = [np.full(t.size, r, np.int32) for r, t in enumerate(ids) if t.size]
    if not owners:
        return np.empty((0, 4), np.int32), np.empty(0, np.int32)
    ids, owners = np.concatenate([t for t in ids if t.size]), np.concatenate(owners)
    ntx = -(-W2 // PASTE_TILE[1])
    order = np.argsort(ids, kind="stable")      # by tile; within a tile the order of the regions stays
    uniq, first, count = np.unique(ids[order], return_index=True, return_counts=True)
    if uniq.size > PASTE_MAX_TILES or ids.size > PASTE_MAX_TILES:
        raise _abi.DpmnError("%s: the regions meet %d tiles (%d list entries), more than fit one launch" % (what, uniq.size, ids.size))
    return np.stack([uniq // ntx, uniq % ntx, first, count], axis=1).astype(np.int32), np.ascontiguousarray(owners[order])


PASTE_KIND_PERSPECTIVE, PASTE_KIND_POLYGON = 0, 1      # csrc/paste_poly.hip KIND_*


def _paste_mixed_plan(photo2, sr_packed, sr_meta, regions, what="paste_mixed_u8", polygons=True):
    """Checks and per-call host data of the paste ops -> host: the arrays of one call as numpy -- table (R, 13) int64 [byte offset of
    the SR image, h_s, w_s, the bits of the float64 feather, kind, then the bits of the 8 float64 coefficients (a quadrilateral) or
    first strip, strip count and zeros (a polygon)], strips (S, 14) int64 [the bits of the 10 float64 of a strip of
    utils.paste_poly.strip_table, its strip_box x0, y0, x1, y1], tiles (n_tiles, 4) int32 [tile row, tile column, first, count] in
    row-major tile order and list (n_list) int32: per tile the regions that meet it, in the order of `regions` -- a quadrilateral
    lies in the tiles that its grown bounding box (utils.paste.region_box) meets, a polygon in those that the box of at least one of
    its strips meets (_paste_mixed_run).  polygons=False (paste_regions_u8): every item must carry 8 coefficients."""
    import numpy as np
    from .utils.paste import region_box
    from .utils.paste_poly import _strips, is_polygon_region, strip_box
    H2, W2, m = _paste_inputs(photo2, sr_packed, sr_meta, what)
    R = len(regions)
    table, strips, n_strips, ids = np.zeros((R, 13), np.int64), [], 0, []
    for r, reg in enumerate(regions):
        try:
            k, shape, feather = reg
            k, feather = int(k), float(feather)
            curved = polygons and is_polygon_region(reg)
            a = _strips(shape, "strips") if curved else np.asarray(shape, np.float64).reshape(-1)
        except (TypeError, ValueError) as e:
            raise _abi.DpmnError("%s: region %d is not (SR index, %s, feather): %s"
                                 % (what, r, "8 coefficients or strips" if polygons else "8 coefficients", e)) from e
        if not (0 <= k < m.shape[0] and (curved or a.size == 8) and np.isfinite(a).all() and np.isfinite(feather)):
            raise _abi.DpmnError("%s: region %d names an SR image outside the batch of %d or does not carry 8 finite coefficients %sand a "
                                 "finite feather" % (what, r, m.shape[0], "(or finite strips) " if polygons else ""))
        table[r, :3] = m[k]
        table[r, 3] = np.float64(feather).view(np.int64)
        if curved:
            boxes = np.array([strip_box(s, H2, W2) for s in a], np.int64)
            table[r, 4:7] = PASTE_KIND_POLYGON, n_strips, a.shape[0]
            strips.append(np.concatenate([np.ascontiguousarray(a).view(np.int64), boxes], axis=1))
            n_strips += a.shape[0]
            ids.append(np.unique(np.concatenate([_box_tile_ids(b, W2) for b in boxes.tolist()])))
        else:
            table[r, 4] = PASTE_KIND_PERSPECTIVE
            table[r, 5:] = a.view(np.int64)
            ids.append(_box_tile_ids(region_box(a, int(m[k, 2]), int(m[k, 1]), H2, W2), W2))
    tiles, lst = _paste_tiles(ids, W2, what)
    return dict(table=table, strips=np.concatenate(strips) if strips else np.empty((0, 14), np.int64), tiles=tiles, list=lst, size=(H2, W2))


def _paste_mixed_run(photo2, sr_packed, host):
    """One upload of the host arrays of _paste_mixed_plan (the region table, the strips, the tiles and the region list in one int64
    buffer) and the launch -> the library's return code."""
    import numpy as np
    table, strips, tiles, lst = (np.ascontiguousarray(host[k], dtype=t) for k, t in
                                 (("table", np.int64), ("strips", np.int64), ("tiles", np.int32), ("list", np.int32)))
    H2, W2 = host["size"]
    if table.shape[0] == 0 or tiles.shape[0] == 0:
        return 0
    d, d_table, d_strips, d_tiles, d_list = _upload(photo2.device, table, strips, tiles, lst)
    return lib.dpmn_paste_mixed_u8(photo2.data_ptr(), H2, W2, sr_packed.data_ptr(), sr_packed.numel(), d_table, table.ctypes.data,
                                   table.shape[0], d_strips, strips.shape[0], d_tiles, tiles.shape[0], d_list, lst.size, stream())


def paste_regions_u8(photo2, sr_packed, sr_meta, regions):
    """The SR regions of one photo pasted back into the enlarged photo (csrc/paste_poly.hip): photo2 a contiguous (H2, W2, 3) uint8 CUDA
    tensor, modified IN PLACE and returned; sr_packed / sr_meta the SR images in utils.resize.pack_ragged's layout (what
    stitch_windows_u8 returns; a contiguous quantize_sr_u8 output viewed flat has it too); regions a list of (SR index, coeffs, feather),
    coeffs the 8 float64 coefficients of utils.paste.paste_coeffs, applied in list order -> byte for byte utils.paste.paste_regions_np,
    in float64.  The host bins the regions into the 8 x 32 tiles of the photo that their grown bounding boxes meet; only those tiles are
    launched, one thread per pixel, so no byte has two owners.  An empty list launches nothing.  Per call one buffer is uploaded: the
    region table, the tiles and the per-tile region list.  paste_mixed_u8 without polygons: an item that carries strips is refused."""
    host = _paste_mixed_plan(photo2, sr_packed, sr_meta, list(regions), what="paste_regions_u8", polygons=False)
    check(_paste_mixed_run(photo2, sr_packed, host))
    return photo2


def paste_mixed_u8(photo2, sr_packed, sr_meta, regions):
    """Quadrilaterals and polygons pasted back into the enlarged photo in one list (csrc/paste_poly.hip): photo2, sr_packed / sr_meta as
    paste_regions_u8 takes them; regions ONE list in paste order whose items are paste_regions_u8's (SR index, coeffs, feather) or
    (SR index, strips, feather) with the float64 (n, 10) strips of utils.paste_poly.strip_table -> byte for byte
    utils.paste_poly.paste_mixed_np, in float64; photo2 is modified IN PLACE and returned.  The tiles, the launch and the one owner per
    byte are paste_regions_u8's; within a polygon a thread tries only the strips whose box holds its pixel.  An empty list launches
    nothing.  Per call one buffer is uploaded: the region table, the strips, the tiles and the per-tile region list."""
    host = _paste_mixed_plan(photo2, sr_packed, sr_meta, list(regions))
    check(_paste_mixed_run(photo2, sr_packed, host))
    return photo2


DETECT_TILE = (16, 64)      # csrc/detect.hip DT_H, DT_W
DETECT_TABLE = 4096         # rows of a photo's component table; a photo with more components gets ONE second pass with as many as it has


def _detect_plan(packed, offsets, sizes, what="detect_text_u8", local=0):
    """Checks and per-call host data of the detect ops -> host: items (B, 8) int64 [byte offset, H, W, offset of the working map, hm, wm,
    r, 0], tiles (n_tiles, 3) int32 [photo, tile row, tile column] over the working maps, map_px: the pixels of all maps.  local (the
    cell side of the locally adaptive threshold, checked here; 0: none): the last word of an item is the offset of the photo's
    ceil(hm / local) x ceil(wm / local) cell thresholds in the batch's table of host["n_cells"] entries -- the cell plan travels with
    the items, in the same upload."""
    import numpy as np
    from .utils.detect import MAP_SIDE, check_local
    try:
        local = check_local(local)
    except ValueError as e:
        raise _abi.DpmnError("%s: %s" % (what, e)) from e
    off = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets)
    sz = np.asarray(sizes.cpu() if torch.is_tensor(sizes) else sizes)
    if off.ndim != 1 or sz.ndim != 2 or sz.shape != (off.shape[0], 2) or off.dtype.kind not in "iu" or sz.dtype.kind not in "iu":
        raise _abi.DpmnError("%s: offsets must be an integer (B) array of byte offsets and sizes an integer (B, 2) array of (h, w)" % what)
    m = _ragged_batch(packed, np.concatenate((off[:, None].astype(np.int64), sz.astype(np.int64)), axis=1), what)
    r = -(-np.maximum(m[:, 1], m[:, 2]) // MAP_SIDE)
    hm, wm = m[:, 1] // r, m[:, 2] // r
    first = np.concatenate(([0], np.cumsum(hm * wm)))
    items = np.zeros((m.shape[0], 8), np.int64)
    items[:, :3], items[:, 3], items[:, 4], items[:, 5], items[:, 6] = m, first[:-1], hm, wm, r
    n_cells = 0
    if local:
        cells = np.concatenate(([0], np.cumsum(-(-hm // local) * -(-wm // local))))
        items[:, 7], n_cells = cells[:-1], int(cells[-1])
    return dict(items=items, tiles=_tile_table(hm, wm, *DETECT_TILE)[0], map_px=int(first[-1]), local=local, n_cells=n_cells)


def _detect_gradient(packed, host, d_items, d_tiles):
    """The gradient launch of one batch -> (g uint8 (map_px), hist int32 (B, 256)) on the device."""
    items, B = host["items"], host["items"].shape[0]
    g = torch.empty(max(host["map_px"], 1), dtype=torch.uint8, device=packed.device)
    hist = torch.empty(B, 256, dtype=torch.int32, device=packed.device)
    check(lib.dpmn_detect_gradient_u8(packed.data_ptr(), packed.numel(), d_items, items.ctypes.data, B, d_tiles, host["tiles"].shape[0],
                                      g.data_ptr(), host["map_px"], hist.data_ptr(), stream()))
    return g, hist


def _detect_thresholds(packed, host, floor):
    """The uploads, the gradient launch, the histogram copy and the thresholds of one batch (utils.detect.threshold, on the host) ->
    (d, d_items, d_tiles, g, hist (host, int64 (B, 256)), thr (device, int32 (B))); d keeps the uploaded buffer alive.
    With host["local"]: no copy and no host step -- the cell-Otsu launch fills thr, the device int32 (n_cells) table of the batch's cell
    thresholds, and hist stays on the device (int32 (B, 256); only detect_maps_u8 copies it)."""
    import numpy as np
    from .utils.detect import threshold
    d, d_items, d_tiles = _upload(packed.device, host["items"], host["tiles"])
    g, hist = _detect_gradient(packed, host, d_items, d_tiles)
    if host["local"]:
        thr = torch.empty(max(host["n_cells"], 1), dtype=torch.int32, device=packed.device)
        check(lib.dpmn_detect_cell_otsu_i32(g.data_ptr(), host["map_px"], d_items, host["items"].ctypes.data, host["items"].shape[0],
                                            host["local"], floor, thr.data_ptr(), host["n_cells"], stream()))
        return d, d_items, d_tiles, g, hist, thr
    hist = hist.cpu().numpy().astype(np.int64)
    thr = torch.from_numpy(np.array([threshold(h, floor) for h in hist], np.int32)).to(packed.device)
    return d, d_items, d_tiles, g, hist, thr


def _detect_label(host, d_items, d_tiles, g, thr, gap, vgap, tmp, smooth, labels, tmap=None):
    """The label launches of one batch: against one threshold per photo, or with host["local"] against the threshold map of the cell
    table thr (tmap: an int32 (map_px) tensor that receives the map)."""
    items, map_px, n_tiles = host["items"], host["map_px"], host["tiles"].shape[0]
    if host["local"]:
        check(lib.dpmn_detect_label_local_i32(g.data_ptr(), map_px, d_items, items.ctypes.data, items.shape[0], d_tiles, n_tiles, thr.data_ptr(),
                                              host["n_cells"], host["local"], gap, vgap, tmp.data_ptr(), smooth.data_ptr(), labels.data_ptr(),
                                              tmap.data_ptr() if tmap is not None else None, stream()))
    else:
        check(lib.dpmn_detect_label_i32(g.data_ptr(), map_px, d_items, items.ctypes.data, items.shape[0], d_tiles, n_tiles, thr.data_ptr(), gap,
                                        vgap, tmp.data_ptr(), smooth.data_ptr(), labels.data_ptr(), stream()))


def _detect_pass(host, d_items, d_tiles, g, thr, gap, vgap):
    """The label and stats launches of one batch over its gradient maps -> dict(smooth, labels, slots: the device maps; slices, d_slices:
    int64 (B, 2) [first row, rows] of every photo's part of the tables; counts (B); table int64 (rows, 5) [x0, y0, greatest x, greatest
    y, area], the rows of a photo in no fixed order).  One copy to the host, the component tables behind their counters; a second, with
    the second pass over the tables, when a photo has more than DETECT_TABLE components."""
    import numpy as np
    items, tiles, map_px, dev = host["items"], host["tiles"], host["map_px"], g.device
    B, n_tiles = items.shape[0], tiles.shape[0]
    tmp, smooth = torch.empty_like(g), torch.empty_like(g)
    labels, slots = torch.empty(g.numel(), dtype=torch.int32, device=dev), torch.empty(g.numel(), dtype=torch.int32, device=dev)
    _detect_label(host, d_items, d_tiles, g, thr, gap, vgap, tmp, smooth, labels)
    caps = np.full(B, DETECT_TABLE, np.int64)
    for _ in range(2):      # (the counters of the first pass are exact: the second pass has a row for every component)
        first = np.concatenate(([0], np.cumsum(caps)))
        slices = np.ascontiguousarray(np.stack((first[:-1], caps), axis=1))
        d_slices = torch.from_numpy(slices).to(dev)
        out = torch.empty(B + int(first[-1]) * 5, dtype=torch.int32, device=dev)      # the counters, then the table: one copy back
        check(lib.dpmn_detect_stats_i32(smooth.data_ptr(), labels.data_ptr(), map_px, d_items, items.ctypes.data, B, d_tiles, n_tiles,
                                        d_slices.data_ptr(), slices.ctypes.data, out.data_ptr(), slots.data_ptr(),
                                        out.data_ptr() + 4 * B, int(first[-1]), stream()))
        out = out.cpu().numpy()
        counts, table = out[:B].astype(np.int64), out[B:].reshape(-1, 5).astype(np.int64)
        if (counts <= caps).all():
            break
        caps = np.maximum(caps, counts)
    else:
        raise _abi.DpmnError("detect: the component counters of two passes over the same labels disagree")
    return dict(smooth=smooth, labels=labels, slots=slots, slices=slices, d_slices=d_slices, counts=counts, table=table)


def _detect_run(packed, host, gap, vgap, floor):
    """The launches of one batch -> (g, hist (host, int64 (B, 256)), smooth, labels, comps): the maps on the device, flat over the batch
    (host["items"] says where a photo's lies), and per photo the int64 (n, 5) table [x0, y0, x1, y1, area] of its components, ends
    exclusive, in no fixed order.  Two copies to the host: the histograms (the thresholds come from them: utils.detect.threshold) and
    the component tables behind their counters; a third, with the second pass over the tables, when a photo has more than DETECT_TABLE
    components.  With host["local"] the first copy falls away: the thresholds are found on the device and hist stays there."""
    d, d_items, d_tiles, g, hist, thr = _detect_thresholds(packed, host, floor)
    p = _detect_pass(host, d_items, d_tiles, g, thr, gap, vgap)
    return g, hist, p["smooth"], p["labels"], _detect_comps(p)


def _detect_comps(p):
    """Per photo the int64 (n, 5) table [x0, y0, x1, y1, area] of a pass of _detect_pass, ends exclusive, in the order of its rows."""
    import numpy as np
    first = p["slices"][:, 0]
    return [p["table"][first[b]:first[b] + n] + np.array([0, 0, 1, 1, 0]) for b, n in enumerate(p["counts"].tolist())]


def _detect_oriented_args(host, d_items, d_tiles, p):
    """The tables of the oriented launches hold exactly the components of a pass, photo after photo: a component's row is its slot of
    _detect_pass behind the components of the photos before it, so only rows that are used are initialised and copied.  -> (the
    leading arguments that the two entry points share, slices int64 (B, 2) [first row, rows], their device copy, the rows in all)."""
    import numpy as np
    items, counts = host["items"], p["counts"]
    first = np.concatenate(([0], np.cumsum(counts)))
    slices = np.ascontiguousarray(np.stack((first[:-1], counts), axis=1))
    d_slices = torch.from_numpy(slices).to(p["smooth"].device)
    args = (p["smooth"].data_ptr(), p["labels"].data_ptr(), host["map_px"], d_items, items.ctypes.data, items.shape[0], d_tiles,
            host["tiles"].shape[0], d_slices.data_ptr(), slices.ctypes.data, p["slots"].data_ptr())
    return args, slices, d_slices, int(first[-1])


def _detect_moments(args, rows, dev):
    """The moments launch and its copy -> int64 (rows, 5) on the host."""
    mom = torch.empty(rows, 5, dtype=torch.int64, device=dev)
    check(lib.dpmn_detect_moments_i64(*args, mom.data_ptr(), rows, stream()))
    return mom.cpu().numpy()


def _detect_dirs(comps, mom, slices):
    """The host's step between the two launches: per photo (comps (n, 5), moments (n, 6), k (n)) -- every component's direction
    (utils.detect.axis_index, in Python ints; -1 where utils.detect.prefilter passes it over) -- and the int32 (rows, 2) table of
    (c, s) that the extents launch reads, (0, 0) for k = -1."""
    import numpy as np
    from .utils.detect import DIRS, axis_index, prefilter
    out, dirs = [], np.zeros((len(mom), 2), np.int32)
    table = np.array(DIRS + ((0, 0),), np.int32)
    for b, c in enumerate(comps):
        at = int(slices[b, 0])
        m = np.concatenate((c[:, 4:5], mom[at:at + len(c)]), axis=1)
        ok = prefilter(c)
        ks = np.full(len(c), -1, np.int64)
        ks[ok] = axis_index(m[ok])
        dirs[at:at + len(c)] = table[ks]
        out.append((c, m, ks))
    return out, dirs


def _detect_extents(args, rows, dirs, dev):
    """The upload of the directions, the extents launch and its copy -> int64 (rows, 4) [U2min, U2max, V2min, V2max] on the host (the
    kernel keeps max -U2, max U2, max -V2, max V2)."""
    import numpy as np
    d_dirs = torch.from_numpy(dirs).to(dev)
    ext = torch.empty(rows, 4, dtype=torch.int32, device=dev)
    check(lib.dpmn_detect_extents_i32(*args, d_dirs.data_ptr(), ext.data_ptr(), rows, stream()))
    return ext.cpu().numpy().astype(np.int64) * np.array([-1, 1, -1, 1])


def _detect_oriented_pass(host, d_items, d_tiles, p):
    """The two oriented launches behind one pass of _detect_pass -> per photo (comps (n, 5), moments (n, 6), k (n), extents (n, 4)) as
    utils.detect's components / moments / axis_index / extents give them, in the order of the photo's table rows.  Two copies to the
    host, the moment table and the extents, each of exactly the components' rows; between them the host chooses the directions."""
    dev = p["smooth"].device
    args, slices, d_slices, rows = _detect_oriented_args(host, d_items, d_tiles, p)
    tables, dirs = _detect_dirs(_detect_comps(p), _detect_moments(args, rows, dev), slices)
    ext = _detect_extents(args, rows, dirs, dev)
    res = []
    for b, (c, m, ks) in enumerate(tables):
        at = int(slices[b, 0])
        e = ext[at:at + len(c)].copy()
        e[ks < 0] = 0
        res.append((c, m, ks, e))
    return res


def _detect_oriented_run(packed, offsets, sizes, gap, vgap, floor, what, local=0):
    """The checks and launches of the oriented ops -> (host, [row pass, column pass]): per pass (what _detect_pass returns, what
    _detect_oriented_pass returns).  One gradient launch and one histogram copy -- with local one cell table -- serve both passes."""
    from .utils.detect import check_params
    try:
        gap, vgap, floor = check_params(gap, vgap, floor)
    except ValueError as e:
        raise _abi.DpmnError("%s: %s" % (what, e)) from e
    host = _detect_plan(packed, offsets, sizes, what, local)
    d, d_items, d_tiles, g, hist, thr = _detect_thresholds(packed, host, floor)
    passes = []
    for a, b in ((gap, vgap), (vgap, gap)):      # the row pass, then the column pass: the same kernels with the gaps swapped
        p = _detect_pass(host, d_items, d_tiles, g, thr, a, b)
        passes.append((p, _detect_oriented_pass(host, d_items, d_tiles, p)))
    return host, passes


def detect_oriented_u8(packed, offsets, sizes, gap=12, vgap=2, floor=24, names=None, local=0):
    """The ORIENTED text regions of a ragged batch of photos (csrc/detect.hip; utils/detect.py holds the recipe): the arguments of
    detect_text_u8 -> per photo an int64 (n, 8) numpy array of quads tl, tr, br, bl (x, y) in hundredths of a photo pixel, not clamped
    to the photo, at most utils.detect.MAX_BOXES: row for row utils.detect.detect_oriented_np.  Two passes over one gradient map and one
    threshold (the smoothing with its gaps as given, then swapped); per pass the components' second moments and, along the direction
    the host chooses from them, their extents.  Integer kernels: the same in every compute mode.  Beyond detect_text_u8's copies, the
    moment tables and the extents of each pass cross to the host.  local: as detect_text_u8 takes it."""
    from .utils.detect import cross_pass, oriented_rects, quads_from_rects
    import numpy as np
    host, passes = _detect_oriented_run(packed, offsets, sizes, gap, vgap, floor, "detect_oriented_u8", local)
    out = []
    for b, it in enumerate(host["items"]):
        H, W = int(it[1]), int(it[2])
        rows, cols = (oriented_rects(c, ks, e, H, W, column) for column, (c, m, ks, e) in ((False, passes[0][1][b]), (True, passes[1][1][b])))
        out.append(quads_from_rects(cross_pass(rows, cols), H, W, names[b] if names else None))
    return out


def detect_oriented_tables_u8(packed, offsets, sizes, gap=12, vgap=2, floor=24, local=0):
    """The tables behind detect_oriented_u8, for tests: per photo [row pass, column pass], each (moments int64 (n, 6), k int64 (n),
    extents int64 (n, 4)) in LABEL order (the labels and slots of every pass are copied back to find it): what
    utils.detect.oriented_pass_np returns first."""
    import numpy as np
    host, passes = _detect_oriented_run(packed, offsets, sizes, gap, vgap, floor, "detect_oriented_tables_u8", local)
    out = [[] for _ in host["items"]]
    for p, tables in passes:
        labels, slots = p["labels"].cpu().numpy(), p["slots"].cpu().numpy()
        for b, (_, _, _, at, hm, wm, _, _) in enumerate(host["items"].tolist()):
            lab = labels[at:at + hm * wm]
            roots = np.nonzero(lab == np.arange(hm * wm))[0]      # ascending: the label order
            order = slots[at:at + hm * wm][roots]
            c, m, ks, e = tables[b]
            out[b].append((m[order], ks[order], e[order]))
    return out


def _detect_profiles(args, rows, bins, dev):
    """The upload of the bins, the profile launch and its copy -> int64 (rows, 16, 4) [top, bot, cnt, sy] on the host, as
    utils.detect.curve_profile gives them (the kernel keeps max -y, max y, count, sum y), zeros where a bin was not used."""
    import numpy as np
    d_bins = torch.from_numpy(bins).to(dev)
    prof = torch.empty(rows, 16, 4, dtype=torch.int32, device=dev)
    check(lib.dpmn_detect_profile_i32(*args, d_bins.data_ptr(), prof.data_ptr(), rows, stream()))
    prof = prof.cpu().numpy().astype(np.int64)
    used = prof[:, :, 2] > 0
    prof[:, :, 0], prof[:, :, 1] = -prof[:, :, 0], prof[:, :, 1] + 1
    prof[~used] = 0
    return prof


def _detect_curved_run(packed, offsets, sizes, gap, vgap, floor, what, local=0):
    """The checks and launches of the curved ops -> (host, pass, per photo (comps (n, 5), candidates (n, 3), profiles (n, 16, 4) or
    None)) in the order of the photo's table rows: detect_text_u8's launches and copies, then the candidates' bins uploaded
    (utils.detect.curve_candidates on the component tables that are on the host already), one launch and one copy back.  A batch
    without a candidate has neither, and no profiles."""
    import numpy as np
    from .utils.detect import check_params, curve_candidates
    try:
        gap, vgap, floor = check_params(gap, vgap, floor)
    except ValueError as e:
        raise _abi.DpmnError("%s: %s" % (what, e)) from e
    host = _detect_plan(packed, offsets, sizes, what, local)
    d, d_items, d_tiles, g, hist, thr = _detect_thresholds(packed, host, floor)
    p = _detect_pass(host, d_items, d_tiles, g, thr, gap, vgap)
    comps = _detect_comps(p)
    cands = [curve_candidates(c) for c in comps]
    if not any((c[:, 2] > 0).any() for c in cands):
        return host, p, [(c, k, None) for c, k in zip(comps, cands)]
    args, slices, d_slices, rows = _detect_oriented_args(host, d_items, d_tiles, p)
    prof = _detect_profiles(args, rows, np.ascontiguousarray(np.concatenate(cands).astype(np.int32)), g.device)
    return host, p, [(c, k, prof[int(at):int(at) + len(c)]) for c, k, at in zip(comps, cands, slices[:, 0])]


def detect_curved_u8(packed, offsets, sizes, gap=12, vgap=2, floor=24, names=None, local=0):
    """The text regions of a ragged batch of photos with BOWED lines as polygons (csrc/detect.hip: k_detect_profile; utils/detect.py
    holds the recipe and its limits): the arguments of detect_text_u8 -> per photo a list of int64 (m, 2) point arrays (x, y) in
    hundredths of a photo pixel, m = 4 for an upright box and 2 bins for a polygon, at most utils.detect.MAX_BOXES: region for region
    utils.detect.detect_curved_np, and for a photo without a curved component the boxes of detect_text_u8.  Beyond detect_text_u8's
    launches and copies: the bins of the candidate components go up, one launch, and the profile table comes back -- none of the three
    when the batch holds no candidate.  Integer kernels: the same in every compute mode."""
    import numpy as np
    from .utils.detect import regions_from_profiles
    host, p, tables = _detect_curved_run(packed, offsets, sizes, gap, vgap, floor, "detect_curved_u8", local)
    out = []
    for b, (it, (c, k, prof)) in enumerate(zip(host["items"], tables)):
        if prof is None:
            prof = np.zeros((len(c), 16, 4), np.int64)
        out.append(regions_from_profiles(c, k, prof, int(it[1]), int(it[2]), names[b] if names else None))
    return out


def detect_curved_tables_u8(packed, offsets, sizes, gap=12, vgap=2, floor=24, local=0):
    """The tables behind detect_curved_u8, for tests: per photo (candidates int64 (n, 3), profiles int64 (n, 16, 4)) in LABEL order (the
    labels and slots are copied back to find it): utils.detect.curve_candidates and curve_profile.  profiles is None for every photo
    of a batch without a candidate: nothing was launched."""
    import numpy as np
    host, p, tables = _detect_curved_run(packed, offsets, sizes, gap, vgap, floor, "detect_curved_tables_u8", local)
    labels, slots = p["labels"].cpu().numpy(), p["slots"].cpu().numpy()
    out = []
    for (_, _, _, at, hm, wm, _, _), (c, k, prof) in zip(host["items"].tolist(), tables):
        roots = np.nonzero(labels[at:at + hm * wm] == np.arange(hm * wm))[0]      # ascending: the label order
        order = slots[at:at + hm * wm][roots]
        out.append((k[order], None if prof is None else prof[order]))
    return out


def detect_text_u8(packed, offsets, sizes, gap=12, vgap=2, floor=24, names=None, local=0):
    """The text regions of a ragged batch of photos (csrc/detect.hip; utils/detect.py holds the recipe): packed = the device copy of
    utils.resize.pack_ragged's buffer, offsets / sizes = the columns of its meta, integer (B) byte offsets and (B, 2) (h, w) -> per
    photo an int32 (n, 4) numpy array of boxes x0, y0, x1, y1 in photo pixels, ends exclusive, sorted by (top, left, bottom, right), at
    most utils.detect.MAX_BOXES: box for box utils.detect.detect_text_np.  gap / vgap: the longest background run that the smoothing
    fills along a row / a column (1 .. 64), floor: the least threshold on the gradient (1 .. 255).  names: per photo, for the line that
    is printed when boxes are dropped.  Integer kernels: the same in every compute mode.  Only the histograms and the component tables
    cross to the host.  local (0: off; else a cell side 32 .. 1024 on the working map): the locally adaptive threshold of
    utils/detect.py -- Otsu's threshold per cell, found on the device, interpolated between the cell centres; the histograms then stay
    on the device, one copy fewer.  local = 1024 is one cell per photo: the boxes of local = 0."""
    from .utils.detect import boxes_from_components, check_params
    try:
        gap, vgap, floor = check_params(gap, vgap, floor)
    except ValueError as e:
        raise _abi.DpmnError("detect_text_u8: %s" % e) from e
    host = _detect_plan(packed, offsets, sizes, local=local)
    comps = _detect_run(packed, host, gap, vgap, floor)[4]
    return [boxes_from_components(c, int(it[1]), int(it[2]), names[b] if names else None) for b, (c, it) in enumerate(zip(comps, host["items"]))]


def detect_maps_u8(packed, offsets, sizes, gap=12, vgap=2, floor=24, local=0):
    """The maps behind detect_text_u8, for tests: per photo (g uint8 (hm, wm), histogram int64 (256), smoothed map uint8 of 0 / 1,
    labels int32: the least linear index of the pixel's component, -1 on the background) as numpy arrays, byte for byte
    utils.detect.detect_maps_np.  local: as detect_text_u8 takes it (the histogram is the whole map's either way)."""
    import numpy as np
    from .utils.detect import check_params
    try:
        gap, vgap, floor = check_params(gap, vgap, floor)
    except ValueError as e:
        raise _abi.DpmnError("detect_maps_u8: %s" % e) from e
    host = _detect_plan(packed, offsets, sizes, "detect_maps_u8", local)
    g, hist, smooth, labels, _ = _detect_run(packed, host, gap, vgap, floor)
    if torch.is_tensor(hist):
        hist = hist.cpu().numpy().astype(np.int64)
    g, smooth, labels = g.cpu().numpy(), smooth.cpu().numpy(), labels.cpu().numpy()
    out = []
    for b, (_, _, _, at, hm, wm, _, _) in enumerate(host["items"].tolist()):
        cut = lambda a: a[at:at + hm * wm].reshape(hm, wm).copy()
        out.append((cut(g), hist[b], cut(smooth), cut(labels)))
    return out


def detect_thresholds_u8(packed, offsets, sizes, local, floor=24):
    """The thresholds behind detect_text_u8(local=...), for tests: per photo (the cell table int32 (ny, nx), the threshold map int32
    (hm, wm)) as numpy arrays -- utils.detect.cell_thresholds and threshold_map.  The table is what the cell-Otsu launch wrote; the map
    is written by the very launch that thresholds (the local row smoothing, under its test pointer)."""
    from .utils.detect import check_params
    try:
        floor = check_params(floor=floor)[2]
        if not int(local):
            raise ValueError("detect: local 0 has no cell table")
    except ValueError as e:
        raise _abi.DpmnError("detect_thresholds_u8: %s" % e) from e
    host = _detect_plan(packed, offsets, sizes, "detect_thresholds_u8", local)
    d, d_items, d_tiles, g, hist, thr = _detect_thresholds(packed, host, floor)
    tmp, smooth = torch.empty_like(g), torch.empty_like(g)
    labels, tmap = torch.empty(g.numel(), dtype=torch.int32, device=g.device), torch.zeros(g.numel(), dtype=torch.int32, device=g.device)
    _detect_label(host, d_items, d_tiles, g, thr, 1, 1, tmp, smooth, labels, tmap)
    thr, tmap, C = thr.cpu().numpy(), tmap.cpu().numpy(), host["local"]
    return [(thr[c:c + -(-hm // C) * -(-wm // C)].reshape(-(-hm // C), -(-wm // C)).copy(), tmap[at:at + hm * wm].reshape(hm, wm).copy())
            for _, _, _, at, hm, wm, _, c in host["items"].tolist()]


def _region_units_table(first_items, rows, block):
    """One block per `block` sample rows of every item -> int32 (n_units, 2) [item, first row]."""
    import numpy as np
    n = -(-rows // block)
    item = np.repeat(np.arange(len(rows), dtype=np.int64) + first_items, n)
    start = np.cumsum(n) - n
    return np.stack([item, (np.arange(int(n.sum()), dtype=np.int64) - np.repeat(start, n)) * block], axis=1).astype(np.int32)


def _region_plan(regions_a, regions_b):
    """The host half of region_overlap_counts: the unit coordinates, boxes, pair list and block tables of a batch, packed for one
    upload -> dict(host, offsets (verts, regions, pairs, area units, pair units) in int64 words, n_verts, R, P, n_area_units,
    n_pair_units, first, pairs, n_pairs)."""
    import numpy as np
    from .utils import detect_eval as de
    if len(regions_a) != len(regions_b):
        raise _abi.DpmnError("region_overlap_counts: %d and %d photos" % (len(regions_a), len(regions_b)))
    try:
        verts, n_pts, boxes = de.regions_flat([r for photo in zip(regions_a, regions_b) for side in photo for r in side])
    except (ValueError, TypeError) as e:
        raise _abi.DpmnError("region_overlap_counts: %s" % e) from e
    n_side = np.array([[len(a), len(b)] for a, b in zip(regions_a, regions_b)], np.int64).reshape(-1, 2)
    first = np.concatenate(([0], np.cumsum(n_side.reshape(-1)))).astype(np.int64)      # photo p: a from first[2p], b from first[2p + 1]
    pairs = [de.meeting_pairs(boxes[first[2 * p]:first[2 * p + 1]], boxes[first[2 * p + 1]:first[2 * p + 2]]) for p in range(len(n_side))]
    n_pairs = np.array([len(p) for p in pairs], np.int64)
    plan = dict(R=len(n_pts), P=int(n_pairs.sum()), first=first, pairs=pairs, n_pairs=n_pairs)
    if not plan["R"]:
        return plan
    block = int(lib.dpmn_region_block())
    table = np.zeros((plan["R"], 8), np.int32)
    table[:, 0], table[:, 1], table[:, 2:6] = np.cumsum(n_pts) - n_pts, n_pts, boxes
    verts = verts.astype(np.int32)
    gpairs = np.concatenate([p + (first[2 * i], first[2 * i + 1]) for i, p in enumerate(pairs)]) if plan["P"] else np.zeros((0, 2), np.int64)
    ua = _region_units_table(0, de.SUB * (boxes[:, 3] - boxes[:, 1]), block)
    ba, bb = boxes[gpairs[:, 0]], boxes[gpairs[:, 1]]
    ub = _region_units_table(0, de.SUB * (np.minimum(ba[:, 3], bb[:, 3]) - np.maximum(ba[:, 1], bb[:, 1])), block)
    host, offsets = _pack(verts, table, np.ascontiguousarray(gpairs, np.int32), ua, ub)
    plan.update(host=host, offsets=offsets, n_verts=len(verts), n_area_units=len(ua), n_pair_units=len(ub))
    return plan


def _region_launch(plan, d, out):
    """The two launches of region_overlap_counts: d = the uploaded plan["host"], out = int64 (R + P) on the device (areas, then pairs)."""
    o_v, o_r, o_p, o_ua, o_ub = plan["offsets"]
    dp, hp, R, st = d.data_ptr(), plan["host"].ctypes.data, plan["R"], _abi.stream_of(d.device)
    check(lib.dpmn_region_area_u64(dp + 8 * o_v, plan["n_verts"], dp + 8 * o_r, hp + 8 * o_r, R, dp + 8 * o_ua, hp + 8 * o_ua,
                                   plan["n_area_units"], out.data_ptr(), st))
    check(lib.dpmn_region_inter_u64(dp + 8 * o_v, plan["n_verts"], dp + 8 * o_r, hp + 8 * o_r, R, dp + 8 * o_p, hp + 8 * o_p, plan["P"],
                                    dp + 8 * o_ub, hp + 8 * o_ub, plan["n_pair_units"], out.data_ptr() + 8 * R, st))


def region_overlap_counts(regions_a, regions_b, device=None):
    """The overlap counts of a batch of photos (csrc/detect_eval.hip; main.py --demo_eval): regions_a / regions_b hold per photo a list
    of (n, 2) point arrays in pixels (the detections and the ground truth) -> per photo the four arrays of
    utils.detect_eval.region_counts_np -- area_a, area_b uint64, pairs int64 (p, 2) in row-major order, inter uint64 (p) -- equal to it
    with == (region_counts_batch_np is the restatement of the whole call).  The host makes the unit coordinates, the integer boxes and
    from them, with NumPy, the pair list (pairs never cross photos); then one upload, two launches (the areas of all regions, the
    intersections of all pairs) and one device-to-host copy.  A batch without a region launches nothing.  Validated on the host; no
    CPU fallback."""
    import numpy as np
    if not torch.cuda.is_available():
        raise _abi.DpmnError("region_overlap_counts: the regions are counted on the GPU; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _abi.DpmnError("region_overlap_counts: the regions are counted on the GPU (got device %s); there is no CPU fallback" % dev)
    plan = _region_plan(regions_a, regions_b)
    R, first, n_pairs = plan["R"], plan["first"], plan["n_pairs"]
    counts = np.zeros(R + plan["P"], np.uint64)
    if R:
        with torch.cuda.device(dev):
            d = torch.from_numpy(plan["host"]).to(dev)
            out = torch.empty(R + plan["P"], dtype=torch.int64, device=dev)
            _region_launch(plan, d, out)
            counts = out.cpu().numpy().view(np.uint64)      # (synchronous: d and out are done with)
    res, at = [], R
    for p in range(len(n_pairs)):
        res.append((counts[first[2 * p]:first[2 * p + 1]].copy(), counts[first[2 * p + 1]:first[2 * p + 2]].copy(), plan["pairs"][p],
                    counts[at:at + n_pairs[p]].copy()))
        at += int(n_pairs[p])
    return res


def maxpool(x, kh, kw, scale=None, shift=None):
    """nn.MaxPool2d((kh,kw), stride (kh,kw)) over NHWC; scale/shift: the producer's BatchNorm affine + ReLU applied on load."""
    B, H, W, Cc = x.shape
    y = torch.empty(B, H // kh, W // kw, Cc, device=x.device)
    check(lib.dpmn_maxpool_f32(dptr(x), dptr(scale, True), dptr(shift, True), dptr(y), B, H, W, Cc, kh, kw, stream()))
    return y


def stn_fc(x, in_affine, w1t, b1, bn, training, w2, b2):
    """STNHead tail (stn_head.py:94-100) -> (img_feat (B,512), ctrl (B, n_out)).  x: (B,1,W2,C) NHWC, bn: nn.BatchNorm1d holder."""
    B, _, W2, _ = x.shape
    feat = torch.empty(B, 512, device=x.device)
    ctrl = torch.empty(B, w2.shape[0], device=x.device)
    sc, sh = in_affine if in_affine is not None else (None, None)
    check(lib.dpmn_stn_fc_f32(dptr(x), dptr(sc, True), dptr(sh, True), W2, dptr(w1t), dptr(b1), dptr(bn.weight), dptr(bn.bias),
                              dptr(bn.running_mean), dptr(bn.running_var), int(training), float(bn.momentum), float(bn.eps),
                              dptr(w2), dptr(b2), dptr(feat), dptr(ctrl), B, w2.shape[0], stream()))
    return feat, ctrl


def tps_sample(img, ctrl, inverse_kernel, coord_repr, out_hw):
    """TPSSpatialTransformer.forward (tps_spatial_transformer.py:97-112) -> (warped (B,C,H,W), source_coordinate (B,H*W,2))."""
    B, Cc, Hin, Win = img.shape
    H, W = out_hw
    out = torch.empty(B, Cc, H, W, device=img.device)
    src = torch.empty(B, H * W, 2, device=img.device)
    check(lib.dpmn_tps_sample_f32(dptr(img), dptr(ctrl), dptr(inverse_kernel), dptr(coord_repr), dptr(out), dptr(src), B, Cc,
                                  Hin, Win, H, W, ctrl.shape[1], stream()))
    return out, src


def dropout(x, p_elem=0.0, seed_elem=0, p_row=0.0, seed_row=0, row_len=0, res=None, out=None):
    """out = res + x * dropout_mask(p_elem) * droppath_mask(p_row per row_len elements); in place on x unless `out` is given."""
    y = x if out is None else out
    check(lib.dpmn_dropout_f32(dptr(x), dptr(res, True), dptr(y), x.numel(), int(row_len), float(p_elem), int(seed_elem),
                               float(p_row), int(seed_row), stream()))
    return y


def sk_fuse(cat, shortcut, proj_w, proj_b, fc1_w, fc1_b, fc2_w, fc2_b, head_w, head_b, groups):
    """shortcut + SKConv(cat)  (pgrm.py:79-96 + 329) on (B, L, C) tokens."""
    B, L, Cd = cat.shape
    M = B * L
    feats = torch.empty_like(cat)
    parts = (L + 31) // 32
    partial = torch.empty(B * parts, Cd, device=cat.device)
    avec = torch.empty(B, groups, Cd // groups, device=cat.device)
    out = torch.empty_like(cat)
    check(lib.dpmn_sk_proj_f32(dptr(cat), dptr(proj_w), dptr(proj_b), dptr(feats), dptr(partial), M, Cd, stream()))
    check(lib.dpmn_sk_gate_f32(dptr(partial), parts, L, dptr(fc1_w), dptr(fc1_b), dptr(fc2_w), dptr(fc2_b), dptr(avec), B,
                               Cd, groups, fc1_w.shape[0], stream()))
    check(lib.dpmn_sk_select_f32(dptr(cat), dptr(avec), dptr(head_w), dptr(head_b), dptr(feats), dptr(shortcut), dptr(out),
                                 M, L, Cd, groups, stream()))
    return out, avec


def sk_mlp_in_supported(M, L, Cd, groups, N):
    return bool(lib.dpmn_sk_mlp_in_supported(M, L, Cd, groups, N))


def sk_mlp_in(cat, avec, head_w, head_b, feats, shortcut, ln_w, ln_b, fc1_w, fc1_b, L, save=False, eps=1e-5, p_row=0.0, seed_row=0):
    """One launch for x1 = proj_head(sum_g avec_g cat_g) + b + feats + shortcut and y = fc1(LayerNorm(x1)) on (M, C) rows.
    Returns (x1, y) or, save=True (training forward), (x1, y, V, n2).  p_row > 0: DropPath (one draw per sample) on the
    attention branch, x1 = shortcut + m_b (proj_head(...) + b + feats)."""
    M, Cd = cat.shape
    G, N = avec.shape[1], fc1_w.shape[0]
    x1, y = torch.empty_like(cat), torch.empty(M, N, device=cat.device)
    V = torch.empty(M, Cd // G, device=cat.device) if save else None
    n2 = torch.empty_like(cat) if save else None
    check(lib.dpmn_sk_mlp_in_drop_f32(dptr(cat), dptr(avec), dptr(head_w), dptr(head_b), dptr(feats), dptr(shortcut), dptr(x1), dptr(ln_w), dptr(ln_b),
                                      eps, dptr(fc1_w), dptr(fc1_b, True), dptr(y), dptr(V, True), dptr(n2, True), M, L, Cd, G, N, float(p_row),
                                      int(seed_row), stream()))
    return (x1, y, V, n2) if save else (x1, y)


def sk_fuse_mlp_in(cat, shortcut, proj_w, proj_b, fc1_w, fc1_b, fc2_w, fc2_b, head_w, head_b, groups, ln_w, ln_b, mlp_fc1_w, mlp_fc1_b,
                   eps=1e-5):
    """x1 = shortcut + SKConv(cat) and y = Mlp.fc1(LayerNorm2(x1)) (no activation) with the select / proj_head / residual /
    LayerNorm / fc1 part in ONE launch (dpmn_sk_mlp_in_f32; pgrm.py:79-96, 327-331, 31).  Returns (x1, y)."""
    B, L, Cd = cat.shape
    M, N = B * L, mlp_fc1_w.shape[0]
    feats = torch.empty_like(cat)
    parts = (L + 31) // 32
    partial = torch.empty(B * parts, Cd, device=cat.device)
    avec = torch.empty(B, groups, Cd // groups, device=cat.device)
    x1 = torch.empty_like(cat)
    y = torch.empty(B, L, N, device=cat.device)
    check(lib.dpmn_sk_proj_f32(dptr(cat), dptr(proj_w), dptr(proj_b), dptr(feats), dptr(partial), M, Cd, stream()))
    check(lib.dpmn_sk_gate_f32(dptr(partial), parts, L, dptr(fc1_w), dptr(fc1_b), dptr(fc2_w), dptr(fc2_b), dptr(avec), B,
                               Cd, groups, fc1_w.shape[0], stream()))
    check(lib.dpmn_sk_mlp_in_f32(dptr(cat), dptr(avec), dptr(head_w), dptr(head_b), dptr(feats), dptr(shortcut), dptr(x1), dptr(ln_w), dptr(ln_b),
                                 eps, dptr(mlp_fc1_w), dptr(mlp_fc1_b, True), dptr(y), None, None, M, L, Cd, groups, N, stream()))
    return x1, y


def dwconv3x3_gelu(y, w, bias, r):
    B, L, Ch = y.shape
    g = torch.empty_like(y)
    check(lib.dpmn_dwconv3x3_gelu_f32(dptr(y), dptr(w), dptr(bias), dptr(g), B, Ch, r, stream()))
    return g


def pointwise(g, w, bias):
    B, L, Ch = g.shape
    z = torch.empty_like(g)
    check(lib.dpmn_pointwise_f32(dptr(g), dptr(w), dptr(bias), dptr(z), B, Ch, L, stream()))
    return z


def pgrm_tail(tokens, w0, b0, w1, b1, weight_list, residuals, H, W, hidden, patch):
    B, L, Cd = tokens.shape
    mid = torch.empty(B * L * hidden * patch * patch + 16 * (9 * Cd + 32), device=tokens.device)
    out = torch.empty(B, hidden, H * patch, W * patch, device=tokens.device)
    check(lib.dpmn_pgrm_tail_f32(dptr(tokens), dptr(w0), dptr(b0), dptr(w1), dptr(b1), _abi.ptr_array(weight_list),
                                 _abi.ptr_array(residuals), len(residuals), dptr(mid), dptr(out), B, H, W, Cd, hidden,
                                 patch, stream()))
    return out


# ------------------------------------------------------------------------------ conv family
_SPLITK_WS = {}


def splitk_workspace(device, floats=24 << 20):
    """One 96 MB scratch per (device, stream) for split-K partial sums (stream-ordered reuse: every conv consumes it before
    the next launch on the same stream; the two refinement branches run on two streams, interfaces/super_resolution.py)."""
    key = (device.type, device.index, _abi_stream_of(device))
    if key not in _SPLITK_WS:
        _SPLITK_WS[key] = torch.empty(floats, device=device)
    return _SPLITK_WS[key]


_ARRIVE_CNT = {}
ARRIVE_CNT_LEN = 32768      # 128 KB: the in-launch split-K reduction keeps its arrival words one 128-byte line apart
STREAM_K = True      # False: the fixed-split path with its reduce launch (tests / A-B runs)


def _attach_workspace(d, device):
    """split-K scratch + the zero-initialised tile-arrival counters of the stream-K conv launch (include/dpmn_hip.h
    dpmn_conv_desc.arrive_cnt: the kernel leaves them zero), one pair per (device, stream)."""
    ws = splitk_workspace(device)
    d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4
    if not STREAM_K:
        d.arrive_cnt, d.arrive_cnt_len = None, 0
        return
    key = (device.type, device.index, _abi_stream_of(device))
    if key not in _ARRIVE_CNT:
        _ARRIVE_CNT[key] = torch.zeros(ARRIVE_CNT_LEN, dtype=torch.int32, device=device)
    d.arrive_cnt, d.arrive_cnt_len = _ARRIVE_CNT[key].data_ptr(), ARRIVE_CNT_LEN


def cmm_forward(weights, keep, x1, x2, c_img, workspaces):
    """ComplementationModulationModule.forward in eval mode as ONE native call (csrc/cmm_forward.hip).  weights: a filled
    _abi.CmmWeights (keep = the tensors it points to); workspaces: dict (B, H, W, stream) -> activation workspace, owned by the module."""
    import ctypes as _C
    B, _, H, W = x1.shape
    x1, x2 = x1.contiguous().float(), x2.contiguous().float()
    key = (B, H, W, _abi_stream_of(x1.device))
    if key not in workspaces:
        workspaces[key] = torch.empty(lib.dpmn_cmm_workspace_bytes(_C.byref(weights), B) // 4, device=x1.device)
    ws = workspaces[key]
    d = _abi.ConvDesc()
    _attach_workspace(d, x1.device)
    sc = _abi.CmmScratch(d.splitk_ws, d.splitk_ws_bytes, d.arrive_cnt, d.arrive_cnt_len)
    out = torch.empty(B, c_img, H, W, device=x1.device)
    check(lib.dpmn_cmm_forward_f32(_C.byref(weights), dptr(x1), dptr(x2), dptr(out), dptr(ws), ws.numel() * 4, _C.byref(sc), B, stream()))
    return out


def psn_trunk(weights, keep, b1, tp, in_planes, workspaces):
    """SRBs + tail of the frozen PSN (TSRN / TATT trunk) as ONE native call (csrc/psn_forward.hip).  b1: block1's NHWC output,
    tp: TATT's NHWC text-prior map or None; returns the NCHW image (B, in_planes, 2H, 2W)."""
    import ctypes as _C
    B, H, W, _ = b1.shape
    key = (B, H, W, _abi_stream_of(b1.device))
    if key not in workspaces:
        workspaces[key] = torch.empty(lib.dpmn_psn_trunk_workspace_bytes(_C.byref(weights), B, H, W) // 4, device=b1.device)
    ws = workspaces[key]
    d = _abi.ConvDesc()
    _attach_workspace(d, b1.device)
    sc = _abi.CmmScratch(d.splitk_ws, d.splitk_ws_bytes, d.arrive_cnt, d.arrive_cnt_len)
    out = torch.empty(B, in_planes, 2 * H, 2 * W, device=b1.device)
    check(lib.dpmn_psn_trunk_f32(_C.byref(weights), dptr(b1), dptr(tp, True), 0 if tp is None else tp.shape[3], dptr(out), dptr(ws),
                                 ws.numel() * 4, _C.byref(sc), B, H, W, stream()))
    return out


def nchw_to_nhwc(x, cpad=None):
    B, Cc, H, W = x.shape
    cpad = cpad or Cc
    out = torch.empty(B, H, W, cpad, device=x.device)
    check(lib.dpmn_nchw_to_nhwc_f32(dptr(x), dptr(out), B, Cc, H, W, cpad, stream()))
    return out


def nhwc_to_nchw(x):
    B, H, W, Cc = x.shape
    out = torch.empty(B, Cc, H, W, device=x.device)
    check(lib.dpmn_nhwc_to_nchw_f32(dptr(x), dptr(out), B, Cc, H, W, stream()))
    return out


def conv_desc(inputs, k, stride=1, pad=0, dil=1, cout=0, pro_act="none", affine=None, phase=None, geom=None):
    """Geometry part of a dpmn_conv_desc.  geom: optional dict overriding (stride, dil, pad_y, pad_x, Hp, Wp, Hout, Wout,
    ostep, ooy, oox) for the odd-pixel scatter of the dilated stride-2 conv's data gradient."""
    d = _abi.ConvDesc()
    B, Hin, Win, _ = inputs[0].shape
    for i, t in enumerate(inputs):
        d.inp[i] = dptr(t)
        d.cseg[i] = t.shape[3]
        if affine is not None and affine[i] is not None:
            d.in_scale[i], d.in_shift[i] = dptr(affine[i][0]), dptr(affine[i][1])
    kh, kw = (k, k) if isinstance(k, int) else k
    d.B, d.Hin, d.Win, d.KH, d.KW = B, Hin, Win, kh, kw
    if geom is not None:
        for key, val in geom.items():
            setattr(d, key, val)
    elif phase is None:
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        d.stride, d.dil_y, d.dil_x, d.pad_y, d.pad_x = stride, dil, dil, ph, pw
        Ho = (Hin + 2 * ph - dil * (kh - 1) - 1) // stride + 1
        Wo = (Win + 2 * pw - dil * (kw - 1) - 1) // stride + 1
        d.Hp, d.Wp, d.Hout, d.Wout, d.ostep, d.ooy, d.oox = Ho, Wo, Ho, Wo, 1, 0, 0
    else:
        py, px = phase
        d.stride, d.dil_y, d.dil_x, d.pad_y, d.pad_x = 1, -1, -1, -py, -px
        d.Hp, d.Wp, d.Hout, d.Wout, d.ostep, d.ooy, d.oox = Hin, Win, 2 * Hin, 2 * Win, 2, py, px
    d.pro_act, d.Cout = ACT[pro_act], cout
    return d


def _stats_ptr(stats, cout):
    """BatchNorm-statistics accumulator of a conv launch: (32, 2, cout) float64 (or a float32 buffer of twice as many elements
    that is zero: the kernels add into it with fp64 atomics, include/dpmn_hip.h dpmn_conv_desc.stats)."""
    if stats is None:
        return None
    ok = stats.is_cuda and stats.is_contiguous() and stats.data_ptr() % 8 == 0 and (
        (stats.dtype == torch.float64 and stats.numel() >= 64 * cout) or (stats.dtype == torch.float32 and stats.numel() >= 128 * cout))
    if not ok:
        raise _abi.DpmnError("conv2d: stats must be a contiguous CUDA (32, 2, Cout) float64 accumulator")
    return stats.data_ptr()


def conv2d(inputs, wp, bias, cout, k, stride=1, pad=0, dil=1, pro_act="none", epi_act="none", slope=0.0, res=None,
           affine=None, out=None, out_nchw=False, pixel_shuffle=False, stats=None, phase=None, geom=None, out_coff=None, groups=1):
    """inputs: list of 1..3 NHWC tensors (channel-concatenated on the fly).  k: int or (KH, KW).
    phase=(py, px): one output phase of ConvTranspose2d(4,2,1) (k=2, dil=-1, pad=-phase).
    affine: optional list of (scale, shift) per input segment.
    groups=2: wp (2, Cout, Kp) / bias (2, Cout) -- images [B/2, B) are convolved with the second weight set (the CMM's twin
    encoder branches in one launch); falls back to two launches over the batch halves when a half does not fill whole
    128-pixel row tiles."""
    if groups == 2:
        B0, h = inputs[0].shape[0], inputs[0].shape[0] // 2
        d0 = conv_desc(inputs, k, stride, pad, dil, cout, pro_act, affine, phase, geom)
        if B0 % 2 or (h * d0.Hp * d0.Wp) % (64 if h * d0.Hp * d0.Wp <= 512 else 128) or stats is not None or res is not None or out_nchw or pixel_shuffle:
            assert out is None and out_coff is None and B0 % 2 == 0
            outs = [conv2d([t[g * h:(g + 1) * h] for t in inputs], wp[g], None if bias is None else bias[g], cout, k, stride, pad, dil,
                           pro_act, epi_act, slope, None if res is None else res[g * h:(g + 1) * h], affine, None, out_nchw,
                           pixel_shuffle, stats, phase, geom) for g in range(2)]
            return torch.cat(outs, 0)
    d = conv_desc(inputs, k, stride, pad, dil, cout, pro_act, affine, phase, geom)
    if groups == 2:
        assert wp.dim() == 3 and wp.is_contiguous() and (bias is None or (bias.dim() == 2 and bias.is_contiguous()))
        d.groups, d.w_group_stride = 2, wp.shape[1] * wp.shape[2]
    B = d.B
    Ho, Wo = d.Hout, d.Wout
    d.epi_act, d.slope = ACT[epi_act], float(slope)
    d.w, d.bias = dptr(wp), dptr(bias, True)
    d.res = dptr(res, True)
    if out is None:
        if out_nchw:
            out = torch.empty(B, cout, Ho, Wo, device=wp.device)
        elif pixel_shuffle:
            out = torch.empty(B, 2 * Ho, 2 * Wo, cout // 4, device=wp.device)
        else:
            out = torch.empty(B, Ho, Wo, cout, device=wp.device)
    d.out = dptr(out)
    d.out_ld, d.out_coff, d.out_nchw, d.pixel_shuffle = 0, 0, int(out_nchw), int(pixel_shuffle)
    if out_coff is not None:      # write channels [out_coff, out_coff + cout) of a wider NHWC buffer
        d.out_ld, d.out_coff = out.shape[3], int(out_coff)
    d.stats = _stats_ptr(stats, cout)
    _attach_workspace(d, wp.device)
    import ctypes as _C
    check(lib.dpmn_conv2d_nhwc_f32(_C.byref(d), stream()))
    return out


def stack_phase_packs(packs):
    """[(wp, bias)] * 4 from packing.pack_convT_s2k4 -> ((4, Cout, Kp) contiguous, bias) for the phase-fused launch."""
    return torch.stack([p[0] for p in packs]).contiguous(), packs[0][1]


def convT_s2k4(inputs, packs, cout, pro_act="none", affine=None, stats=None):
    """ConvTranspose2d(4, stride 2, padding 1): all 4 output phases in ONE launch (nphase = 4).
    packs: ((4, Cout, Kp) phase-major packed weights, bias or None) -- see stack_phase_packs / packing.tpack_convT_s2k4."""
    if isinstance(packs, list):
        packs = stack_phase_packs(packs)
    wp4, bias = packs
    B, Hin, Win, _ = inputs[0].shape
    out = torch.empty(B, 2 * Hin, 2 * Win, cout, device=inputs[0].device)
    d = conv_desc(inputs, 2, cout=cout, pro_act=pro_act, affine=affine, phase=(0, 0))
    d.nphase, d.w_phase_stride = 4, wp4.shape[1] * wp4.shape[2]
    d.w, d.bias = dptr(wp4), dptr(bias, True)
    d.out, d.stats = dptr(out), _stats_ptr(stats, cout)
    _attach_workspace(d, out.device)
    import ctypes as _C
    check(lib.dpmn_conv2d_nhwc_f32(_C.byref(d), stream()))
    return out


def se_gate(x, fc1_w, fc1_b, fc2_w, fc2_b):
    B, H, W, Cc = x.shape
    out = torch.empty_like(x)
    hid = torch.empty(B, fc1_w.shape[0], device=x.device)
    check(lib.dpmn_se_gate_f32(dptr(x), dptr(fc1_w), dptr(fc1_b), dptr(fc2_w), dptr(fc2_b), dptr(out), dptr(hid), B, H * W,
                               Cc, fc1_w.shape[0], stream()))
    return out


# ------------------------------------------------------------------------------ TSRN / TATT pieces
def bigru(gi, w_hh, b_hh, B, H, W, axis, res=None, hidden=32):
    """gi: NHWC (B,H,W,6*hidden) input projections.  axis='w': sequences run along W (rows as batch);
    axis='h': along H (the transposed gru1 call).  Returns NHWC (B,H,W,2*hidden) (+ res)."""
    out = torch.empty(B, H, W, 2 * hidden, device=gi.device)
    if axis == "w":
        nseq, T, inner, outer, inner_s, step = B * H, W, 1, W, 0, 1
    else:
        nseq, T, inner, outer, inner_s, step = B * W, H, W, H * W, 1, W
    check(lib.dpmn_bigru_f32(dptr(gi), dptr(w_hh), dptr(b_hh), dptr(res, True), dptr(out), nseq, T, inner, outer, inner_s,
                             step, hidden, stream()))
    return out


def small_linear(x, w, b=None, add=None, act="none", slope=0.0):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device)
    check(lib.dpmn_small_linear_f32(dptr(x), dptr(add, True), 0 if add is None else add.shape[0], dptr(w), dptr(b, True),
                                    dptr(y), M, N, K, ACT[act], float(slope), stream()))
    return y


def tatt_encoder_layer(src, pos, w12, nhead=4):
    N, L, E = src.shape
    mem = torch.empty_like(src)
    check(lib.dpmn_tatt_encoder_layer_f32(dptr(src), dptr(pos), _abi.ptr_array(w12), dptr(mem), N, L, E, nhead, stream()))
    return mem


def cross_attn(q, k, v, nhead=4, need_weights=False):
    N, L, E = q.shape
    S = k.shape[1]
    o = torch.empty_like(q)
    pw = torch.empty(N, L, S, device=q.device) if need_weights else None
    check(lib.dpmn_cross_attn_f32(dptr(q), dptr(k), dptr(v), dptr(o), dptr(pw, True), N, L, S, E, nhead, stream()))
    return o, pw


def add_layernorm64(x, res, g, b, g2=None, b2=None, acc_out=None, alpha=1.0, accumulate=False):
    M = x.numel() // 64
    y = torch.empty_like(x)
    check(lib.dpmn_add_layernorm64_f32(dptr(x), dptr(res, True), dptr(g), dptr(b), dptr(y), dptr(g2, True), dptr(b2, True),
                                       dptr(acc_out, True), float(alpha), int(accumulate), M, stream()))
    return y


def cross_attn_qproj(x, qe, wq, bq, k, v, nhead=4, need_weights=False):
    """cross_attn(add_linear(x, qe, wq, bq), k, v) with the q projection inside the attention launch"""
    N, L, E = x.shape
    S = k.shape[1]
    o = torch.empty_like(x)
    pw = torch.empty(N, L, S, device=x.device) if need_weights else None
    check(lib.dpmn_cross_attn_qproj_f32(dptr(x), dptr(qe), dptr(wq), dptr(bq, True), dptr(k), dptr(v), dptr(o), dptr(pw, True),
                                        N, L, S, E, nhead, stream()))
    return o, pw


def tatt_dec_tail(o, res, out_w, out_b, n2_w, n2_b, l1_w, l1_b, l2_w, l2_b, n3_w, n3_b, g2=None, b2=None, acc_out=None, alpha=1.0,
                  accumulate=False):
    """one decoder layer after its cross attention (out_proj + res, norm2, FFN + res, norm3, optional second norm into acc_out)"""
    M = o.numel() // 64
    d = _abi.TattDecLayer()
    for n, t in (("out_w", out_w), ("out_b", out_b), ("norm2_w", n2_w), ("norm2_b", n2_b), ("lin1_w", l1_w), ("lin1_b", l1_b),
                 ("lin2_w", l2_w), ("lin2_b", l2_b), ("norm3_w", n3_w), ("norm3_b", n3_b)):
        setattr(d, n, dptr(t))
    y = torch.empty_like(o)
    check(lib.dpmn_tatt_dec_tail_f32(dptr(o), dptr(res), _abi.C.byref(d), dptr(y), dptr(g2, True), dptr(b2, True), dptr(acc_out, True),
                                     float(alpha), int(accumulate), M, stream()))
    return y


def gru_gate(gi, gh, h, hist, hist_row_stride):
    R, H = h.shape
    check(lib.dpmn_gru_gate_f32(dptr(gi), dptr(gh), dptr(h), hist.data_ptr(), hist_row_stride, R, H, stream()))


# ------------------------------------------------------------------------------ image-space helpers
def _nchw_view(x):
    """(pointer, per-image stride) of an NCHW tensor whose images are contiguous (channel-sliced views allowed)."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise _abi.DpmnError("dpmn_amd: expected a float32 CUDA tensor")
    B, Cc, H, W = x.shape
    if x.stride()[1:] != (H * W, W, 1):
        x = x.contiguous()
    return x, x.data_ptr(), x.stride(0)


def to_mask(img):
    """toMask (utils/util.py:27-35) for a whole batch; img (B,>=3,H,W) -> (B,3,H,W) in {0,1}."""
    img, p, st = _nchw_view(img)
    B, _, H, W = img.shape
    out = torch.empty(B, 3, H, W, device=img.device)
    check(lib.dpmn_to_mask_f32(p, st, dptr(out), B, H, W, stream()))
    return out


def mha32(qkv, B, L, heads, scale):
    """MultiHeadedAttention core of TBSRN (tbsrn.py:110-150): qkv (B*L, 3*heads*32) -> (B*L, heads*32)."""
    out = torch.empty(B * L, heads * 32, device=qkv.device)
    check(lib.dpmn_mha32_f32(dptr(qkv), dptr(out), B, L, heads, float(scale), stream()))
    return out


def layernorm_std(x, a2, b2, eps=1e-6):
    """tbsrn.py:23-36 LayerNorm: a2 * (x - mean) / (unbiased std + eps) + b2 over the last axis of (M, C)."""
    y = torch.empty_like(x)
    check(lib.dpmn_layernorm_std_f32(dptr(x), dptr(a2), dptr(b2), float(eps), dptr(y), x.shape[0], x.shape[1], stream()))
    return y


def rotate_img(img, arc, rand_offs, off_range=0.2):
    """torch_rotate_img (utils/util.py:37-58): img (N,C,H,W), arc / rand_offs (N) -> rotated, aspect-jittered batch."""
    img = img.contiguous().float()
    N, Cc, H, W = img.shape
    out = torch.empty_like(img)
    check(lib.dpmn_rotate_img_f32(dptr(img), dptr(arc.contiguous().float()), dptr(rand_offs.contiguous().float()), float(off_range),
                                  dptr(out), N, Cc, H, W, stream()))
    return out


def blend(a, b, alpha):
    """alpha*a + (1-alpha)*b[:, :C] (super_resolution.py:449)."""
    a, pa, sa = _nchw_view(a)
    b, pb, sb = _nchw_view(b)
    B, Cc, H, W = a.shape
    out = torch.empty(B, Cc, H, W, device=a.device)
    check(lib.dpmn_blend_f32(pa, sa, pb, sb, dptr(out), float(alpha), B, Cc * H * W, stream()))
    return out


def psnr_ssim(x, y):
    """(psnr, ssim) device scalars over the first 3 channels (utils/ssim_psnr.py)."""
    x, px, sx = _nchw_view(x)
    y, py, sy = _nchw_view(y)
    B, _, H, W = x.shape
    ws = torch.empty(lib.dpmn_psnr_ssim_workspace_bytes(B, 3, H, W), dtype=torch.uint8, device=x.device)
    out = torch.empty(2, device=x.device)
    check(lib.dpmn_psnr_ssim_f32(px, sx, py, sy, dptr(out), ws.data_ptr(), B, 3, H, W, stream()))
    return out[0], out[1]


# ------------------------------------------------------------------ in-loop text prior (csrc/visionlan.hip)
def mha64(qkv, B, L, heads, scale):
    """VisionLAN MultiHeadAttention core (modules.py:43-81): qkv (B*L, 3*heads*64) rows [q|k|v] -> (B*L, heads*64)."""
    out = torch.empty(B * L, heads * 64, device=qkv.device)
    check(lib.dpmn_mha64_f32(dptr(qkv), dptr(out), B, L, heads, float(scale), stream()))
    return out


def layernorm(x, w, b, eps=1e-5):
    """nn.LayerNorm over the last axis of (M, C), C in {64, 96, 192, 512}."""
    y = torch.empty_like(x)
    check(lib.dpmn_layernorm_f32(dptr(x), dptr(w), dptr(b), float(eps), dptr(y), x.shape[0], x.shape[1], stream()))
    return y


def act(x, kind):
    y = torch.empty_like(x)
    check(lib.dpmn_act_fwd_f32(dptr(x), dptr(y), ACT[kind], 0.0, x.numel(), stream()))
    return y


def vl_resize(img, out_h=64, out_w=256):
    """parse_visionlan_data (base.py:473-478) for a batch: (B, >=3, H, W) -> NHWC (B, out_h, out_w, 4), channel 3 zero."""
    B, _, H, W = img.shape
    v, ptr, stride = _nchw_view(img)
    out = torch.empty(B, out_h, out_w, 4, device=img.device)
    check(lib.dpmn_vl_resize_f32(ptr, stride, dptr(out), B, H, W, out_h, out_w, stream()))
    return out


def vl_tokens(feat, pos_table):
    B, Hf, Wf, Cc = feat.shape
    tok = torch.empty(B, Hf * Wf, Cc, device=feat.device)
    check(lib.dpmn_vl_tokens_f32(dptr(feat), dptr(pos_table), dptr(tok), B, Hf, Wf, Cc, stream()))
    return tok


def vl_pp_pool(scores, enc, w_vrm, b_vrm, n_steps):
    B, L, Cc = enc.shape
    n_class = w_vrm.shape[0]
    logits = torch.empty(B, n_steps, n_class, device=enc.device)
    check(lib.dpmn_vl_pp_pool_f32(dptr(scores), scores.shape[1], dptr(enc), dptr(w_vrm), dptr(b_vrm), dptr(logits), B, L, Cc, n_steps,
                                  n_class, stream()))
    return logits


def vl_decode(logits, max_len=25):
    B, n_steps, n_class = logits.shape
    cls = torch.empty(B, max_len, dtype=torch.int32, device=logits.device)
    length = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib.dpmn_vl_decode_i32(dptr(logits), cls.data_ptr(), length.data_ptr(), B, n_steps, n_class, max_len, stream()))
    return cls, length


def text_prior_compose(cls, length, atlas, advance, out_h, out_w):
    """cls (B, max_len) int32, length (B) int32, atlas (2, n_glyph, GH, GW) float 0..255, advance (2, n_glyph) int32."""
    B, max_len = cls.shape
    _, n_glyph, GH, GW = atlas.shape
    out = torch.empty(B, 2, out_h, out_w, device=atlas.device)
    for t_ in (cls, length, advance):
        if not (t_.is_cuda and t_.dtype == torch.int32 and t_.is_contiguous()):
            raise _abi.DpmnError("dpmn_amd: text_prior_compose expects contiguous int32 CUDA index tensors")
    check(lib.dpmn_text_prior_compose_f32(cls.data_ptr(), length.data_ptr(), dptr(atlas), advance.data_ptr(), dptr(out), B, max_len,
                                          n_glyph, GH, GW, out_h, out_w, stream()))
    return out


# ------------------------------------------------------------------------------ native CRNN recogniser (csrc/crnn.hip)
def _gray_prep(name, img, out_h, out_w, with_plane):
    B, Cc, H, W = img.shape
    if Cc < 3:
        raise _abi.DpmnError("%s: channels 0..2 (RGB) are read, got %d channels" % (name, Cc))
    v, ptr, stride = _nchw_view(img)
    plane = torch.empty(B, 1, out_h, out_w, device=img.device) if with_plane else None
    out = torch.empty(B, out_h, out_w, 4, device=img.device)
    check(lib.dpmn_gray_prep_f32(ptr, stride, dptr(plane, allow_none=True), dptr(out), B, H, W, out_h, out_w, stream()))
    return plane, out


def crnn_prep(img, out_h=32, out_w=100):
    """parse_crnn_data (base.py:419-425) for a batch: (B, >=3, H, W) -> NHWC (B, out_h, out_w, 4), channel 0 = luma, 1..3 zero."""
    return _gray_prep("crnn_prep", img, out_h, out_w, False)[1]


def maxpool2d(x, k, stride, pad=(0, 0)):
    """nn.MaxPool2d(k, stride, pad) over NHWC (B, H, W, C); k, stride, pad are (y, x) pairs."""
    B, H, W, Cc = x.shape
    Ho, Wo = (H + 2 * pad[0] - k[0]) // stride[0] + 1, (W + 2 * pad[1] - k[1]) // stride[1] + 1
    y = torch.empty(B, Ho, Wo, Cc, device=x.device)
    check(lib.dpmn_maxpool2d_f32(dptr(x), dptr(y), B, H, W, Cc, k[0], k[1], stride[0], stride[1], pad[0], pad[1], stream()))
    return y


def bilstm(gx, w_hh, B, T):
    """Recurrence of a bidirectional nn.LSTM with hidden 256: gx (B*T, 2048) input projection + both biases (row b*T + t,
    columns [forward i f g o | backward i f g o]), w_hh (2, 1024, 256) -> (B*T, 512) = [h_fwd | h_bwd]."""
    Hd = w_hh.shape[2]
    if tuple(gx.shape) != (B * T, 8 * Hd) or tuple(w_hh.shape) != (2, 4 * Hd, Hd):
        raise _abi.DpmnError("bilstm: gx (B*T, 8H) and w_hh (2, 4H, H) expected, got %s, %s" % (tuple(gx.shape), tuple(w_hh.shape)))
    out = torch.empty(B * T, 2 * Hd, device=gx.device)
    c = torch.empty(2, B, Hd, device=gx.device)
    check(lib.dpmn_bilstm_f32(dptr(gx), dptr(w_hh), dptr(out), dptr(c), B, T, Hd, stream()))
    return out


def ctc_greedy(logits, B, T, n_class, extra=0):
    """logits rows b*T + t (B*T, ld) -> one int32 buffer (B*T + B): cls (B, T) collapsed classes then length (B); returned as
    (buffer, cls view, length view) so that the host reads both with one copy.  extra: that many more int32 at the end of the
    buffer, for a caller that wants further results in the same copy (ctc_lexicon's `out`)."""
    if logits.dim() != 2 or logits.shape[0] != B * T or logits.shape[1] < n_class:
        raise _abi.DpmnError("ctc_greedy: logits rows (B*T, >= n_class) expected")
    buf = torch.empty(B * T + B + extra, dtype=torch.int32, device=logits.device)
    check(lib.dpmn_ctc_greedy_i32(dptr(logits), logits.shape[1], n_class, buf.data_ptr(), buf.data_ptr() + 4 * B * T, B, T, stream()))
    return buf, buf[:B * T].view(B, T), buf[B * T:B * T + B]


def crnn_label_vecs(logits, B, T, n_class):
    """softmax over the classes of logits rows b*T + t (B*T, ld) -> (B, n_class, 1, T)."""
    if logits.dim() != 2 or logits.shape[0] != B * T or logits.shape[1] < n_class:
        raise _abi.DpmnError("crnn_label_vecs: logits rows (B*T, >= n_class) expected")
    out = torch.empty(B, n_class, 1, T, device=logits.device)
    check(lib.dpmn_crnn_label_vecs_f32(dptr(logits), logits.shape[1], n_class, dptr(out), B, T, stream()))
    return out


# ------------------------------------------------------------------------------ lexicon-constrained reading (csrc/lexicon.hip)
class Lexicon:
    """A word list for lexicon-constrained reading (utils/lexicon.py): `words` (distinct strings over `alphabet`, default the
    CRNN's), `packed` their (L, 32) uint8 records.  The records are uploaded once per device and the kernels' workspace is kept per
    (device, stream).  mode: None (the recogniser's own protocol: CTC score for the CRNN, edit distance for the others), 'score' or
    'edit' (main.py --rec_lexicon_mode)."""

    def __init__(self, words, alphabet=None, mode=None):
        from .utils import lexicon as lx
        if mode not in (None, "score", "edit"):
            raise ValueError("Lexicon: mode is None, 'score' or 'edit', got %r" % (mode,))
        self.words = list(words)
        if not 1 <= len(self.words) <= lx.MAX_WORDS:
            raise ValueError("Lexicon: 1 .. %d words are supported, got %d" % (lx.MAX_WORDS, len(self.words)))
        self.alphabet = alphabet
        self.packed = lx.pack_lexicon(self.words, alphabet)
        self.max_class = int(self.packed[:, 1:].max())
        self.mode = mode
        self._dev, self._ws = {}, {}
        self._trie, self._trie_dev = None, {}

    @property
    def trie(self):
        """The prefix trie of the words (utils.line_words.build_trie: an (N, 4) int32 table), built on first use."""
        if self._trie is None:
            from .utils.line_words import build_trie
            self._trie = build_trie(self.packed)
        return self._trie

    def device_trie(self, device):
        """The trie on `device` (a flat int32 tensor of 4 N entries), uploaded on first use."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _abi.DpmnError("Lexicon: the lexicon kernels run on the GPU only (got %s); there is no CPU fallback" % device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        t = self._trie_dev.get(key)
        if t is None:
            t = self._trie_dev[key] = torch.from_numpy(self.trie.reshape(-1)).to(torch.device("cuda", key))
        return t

    @classmethod
    def from_file(cls, path, voc_type="lower", mode=None):
        from .utils import lexicon as lx
        return cls(lx.load_lexicon(path, voc_type), mode=mode)

    def __len__(self):
        return len(self.words)

    def device_words(self, device):
        """The records on `device` (a flat uint8 tensor of 32 L bytes), uploaded on first use."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _abi.DpmnError("Lexicon: the lexicon kernels run on the GPU only (got %s); there is no CPU fallback" % device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = torch.from_numpy(self.packed.reshape(-1)).to(torch.device("cuda", key))
        return t

    def workspace(self, device, nbytes):
        """At least nbytes of scratch on `device` for the current stream (kept; grown when a larger batch comes)."""
        device = torch.device(device)
        key = (device.index if device.index is not None else torch.cuda.current_device(), _abi.stream_of(device))
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = self._ws[key] = torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=device)
        return t

    def strings(self, idx):
        """word indices (-1: no word) -> strings ('' for -1)"""
        return [self.words[i] if i >= 0 else "" for i in (int(v) for v in idx)]


def _lex_out(out, B, device, what):
    if out is None:
        return torch.empty(2 * B, dtype=torch.int32, device=device)
    if not (torch.is_tensor(out) and out.device == device and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == 2 * B):
        raise _abi.DpmnError("%s: out must be a contiguous int32 tensor of 2 B elements on %s" % (what, device))
    return out


def ctc_lexicon(logits, B, T, n_class, lex, out=None):
    """The lexicon word of the highest CTC likelihood per image: logits rows b*T + t (B*T, ld >= n_class; logits_rows' layout, the
    padding columns are not read), lex a Lexicon -> one int32 buffer (2 B): the word indices (B; -1 when no word fits T frames),
    then the bits of the float32 log-likelihoods (B; -inf with -1): `buf[B:].view(torch.float32)`.  out: write into this int32
    tensor of 2 B elements instead (ctc_greedy's `extra`)."""
    if not isinstance(lex, Lexicon):
        raise _abi.DpmnError("ctc_lexicon: lex must be an ops.Lexicon")
    if logits.dim() != 2 or logits.shape[0] != B * T or logits.shape[1] < n_class:
        raise _abi.DpmnError("ctc_lexicon: logits rows (B*T, >= n_class) expected")
    if lex.max_class >= n_class:
        raise _abi.DpmnError("ctc_lexicon: the lexicon holds class %d, the logits have %d classes" % (lex.max_class, n_class))
    words = lex.device_words(logits.device)
    L = len(lex)
    out = _lex_out(out, B, logits.device, "ctc_lexicon")
    ws = lex.workspace(logits.device, lib.dpmn_ctc_lexicon_workspace_bytes(B, L))
    check(lib.dpmn_ctc_lexicon_f32(dptr(logits), logits.shape[1], n_class, words.data_ptr(), L, out.data_ptr(), out.data_ptr() + 4 * B,
                                   ws.data_ptr(), B, T, stream()))
    return out


def edit_lexicon(strings_packed, lex, out=None):
    """The lexicon word at the least Levenshtein distance per string: strings_packed a (B, 32) uint8 CUDA tensor of records
    (utils.lexicon.pack_strings; length 0 allowed), lex a Lexicon -> one int32 buffer (2 B): the word indices, then the distances."""
    if not isinstance(lex, Lexicon):
        raise _abi.DpmnError("edit_lexicon: lex must be an ops.Lexicon")
    s = strings_packed
    if not (torch.is_tensor(s) and s.is_cuda and s.dtype == torch.uint8 and s.dim() == 2 and s.shape[1] == 32 and s.is_contiguous()
            and s.shape[0] > 0):
        raise _abi.DpmnError("edit_lexicon: a contiguous (B, 32) uint8 CUDA tensor of packed strings is required; there is no CPU fallback")
    B, L = s.shape[0], len(lex)
    words = lex.device_words(s.device)
    out = _lex_out(out, B, s.device, "edit_lexicon")
    ws = lex.workspace(s.device, lib.dpmn_edit_lexicon_workspace_bytes(B, L))
    check(lib.dpmn_edit_lexicon_i32(s.data_ptr(), words.data_ptr(), L, out.data_ptr(), out.data_ptr() + 4 * B, ws.data_ptr(), B, stream()))
    return out


def edit_read(strings, lex, device):
    """The edit protocol for a recogniser's strings: packed on the host (utils.lexicon.pack_strings, under the lexicon's alphabet),
    uploaded, dpmn_edit_lexicon_i32, ONE copy back -> (the lexicon's words, the distances), one per string."""
    from .utils import lexicon as lx
    if not len(strings):
        return [], []
    packed = torch.from_numpy(lx.pack_strings(strings, lex.alphabet)).to(device)
    h = edit_lexicon(packed, lex).cpu().numpy()
    B = len(strings)
    return lex.strings(h[:B]), [int(d) for d in h[B:]]


# ------------------------------------------------------------------------------ CTC beam search with a character model (csrc/beam.hip)
class CharLM:
    """A character n-gram model for ctc_beam (utils/beam.py): `table`, the float32 natural logs (37 ** (order - 1), 37) of
    utils.beam.build_char_lm, and its `order` (1 .. 3).  The table is uploaded once per device and kept."""

    def __init__(self, table, order):
        import numpy as np
        from .utils import beam as bm
        table = np.ascontiguousarray(table)
        if order not in (1, 2, 3) or bm.table_order(table) != order:
            raise _abi.DpmnError("CharLM: order is 1 .. %d and the table float32 (37 ** (order - 1), 37), got order %r and %s %s"
                                 % (bm.MAX_ORDER, order, table.dtype, table.shape))
        if not np.isfinite(table).all():
            raise _abi.DpmnError("CharLM: the table holds a value that is not finite")
        self.table, self.order = table, int(order)
        self.uploads = 0
        self._dev = {}

    @classmethod
    def from_file(cls, path, voc_type="lower", order=3, k=4.0):
        """The model of a word file (utils.beam.load_lm_words: the lexicon loader's filter, duplicates count)."""
        from .utils import beam as bm
        if order not in (1, 2, 3):
            raise _abi.DpmnError("CharLM: order is 1 .. %d, got %r" % (bm.MAX_ORDER, order))
        return cls(bm.build_char_lm(bm.load_lm_words(path, voc_type), order, k), order)

    def device_table(self, device):
        """The table on `device` (a flat float32 tensor), uploaded on first use (`uploads` counts them)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _abi.DpmnError("CharLM: the beam search runs on the GPU only (got %s); there is no CPU fallback" % device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = torch.from_numpy(self.table.reshape(-1)).to(torch.device("cuda", key))
            self.uploads += 1
        return t


def ctc_beam(logits, B, T, n_class, lm=None, width=16, alpha=0.5, beta=0.0, out=None):
    """The CTC prefix beam search of utils/beam.py per image, in ONE launch: logits rows b*T + t (B*T, >= n_class) float32 with unit
    column stride (logits_rows' layout or a column slice of it; the columns at or beyond n_class are not read), lm a CharLM or None
    (alpha then counts as 0), width 1 .. 32, alpha the model's weight, beta added per symbol -> one int32 buffer (B*T + 3 B): the
    classes of the best prefix (B, T) zero-filled, the lengths (B), then the bits of the float64 scores (B):
    `buf[B*T + B:].view(torch.float64)` on the host copy.  out: write into this int32 tensor of B*T + 3 B elements instead
    (ctc_greedy's `extra`).  T <= 64, n_class <= 64 (<= 37 with a model); DpmnError outside the limits."""
    import math
    from .utils import beam as bm
    if lm is not None and not isinstance(lm, CharLM):
        raise _abi.DpmnError("ctc_beam: lm must be an ops.CharLM or None")
    if not (torch.is_tensor(logits) and logits.is_cuda):
        raise _abi.DpmnError("ctc_beam: the beam search runs on the GPU only (got a %s tensor); there is no CPU fallback"
                             % (logits.device if torch.is_tensor(logits) else type(logits).__name__))
    if (logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[0] != B * T or logits.shape[1] < n_class or B < 1
            or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]):
        raise _abi.DpmnError("ctc_beam: float32 logits rows (B*T, >= n_class) with unit column stride expected")
    if not (1 <= T <= bm.MAX_T and 2 <= n_class <= bm.MAX_CLASS):
        raise _abi.DpmnError("ctc_beam: 1 .. %d frames and 2 .. %d classes are supported, got T = %d, n_class = %d"
                             % (bm.MAX_T, bm.MAX_CLASS, T, n_class))
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= bm.MAX_WIDTH:
        raise _abi.DpmnError("ctc_beam: the width is an integer 1 .. %d, got %r" % (bm.MAX_WIDTH, width))
    if not (math.isfinite(float(alpha)) and math.isfinite(float(beta))):
        raise _abi.DpmnError("ctc_beam: alpha and beta must be finite, got %r, %r" % (alpha, beta))
    if lm is not None and n_class > bm.LM_CLASSES:
        raise _abi.DpmnError("ctc_beam: the model knows %d classes, the logits have %d" % (bm.LM_CLASSES, n_class))
    n = B * T + 3 * B
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=logits.device)
    elif not (torch.is_tensor(out) and out.device == logits.device and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == n):
        raise _abi.DpmnError("ctc_beam: out must be a contiguous int32 tensor of B*T + 3 B elements on %s" % logits.device)
    table = lm.device_table(logits.device) if lm is not None else None
    p = out.data_ptr()
    with torch.cuda.device(logits.device):
        check(lib.dpmn_ctc_beam_f64(logits.data_ptr(), logits.stride(0), n_class, table.data_ptr() if table is not None else None,
                                    lm.order if lm is not None else 0, width, float(alpha), float(beta), p, p + 4 * B * T,
                                    p + 4 * (B * T + B), B, T, stream()))
    return out


def ctc_beam_decode(h, B, T):
    """The host half: h = ctc_beam's buffer as a NumPy int32 array -> (classes (B, T), lengths (B), float64 scores (B))."""
    import numpy as np
    h = np.ascontiguousarray(h)
    return h[:B * T].reshape(B, T), h[B * T:B * T + B], h[B * T + B:B * T + 3 * B].copy().view(np.float64)


# ------------------------------------------------------------------------------ recogniser confidence (csrc/confidence.hip)
def ctc_confidence(logits, B, T, n_class, buf):
    """The CTC log-likelihood of every image's own greedy string (utils.confidence.ctc_score): logits rows b*T + t (B*T, ld >=
    n_class; the padding columns are not read), buf = ctc_greedy's buffer made with extra >= B.  The float32 score bits go behind
    the lengths, `buf[B*T + B:B*T + 2*B].view(torch.float32)` (returned), so that one copy of buf brings string and score."""
    if logits.dim() != 2 or logits.shape[0] != B * T or logits.shape[1] < n_class:
        raise _abi.DpmnError("ctc_confidence: logits rows (B*T, >= n_class) expected")
    if not (torch.is_tensor(buf) and buf.device == logits.device and buf.dtype == torch.int32 and buf.is_contiguous()
            and buf.dim() == 1 and buf.numel() >= B * T + 2 * B):
        raise _abi.DpmnError("ctc_confidence: buf must be ops.ctc_greedy's int32 buffer with extra >= B")
    n = B * T
    check(lib.dpmn_ctc_conf_f32(dptr(logits), logits.shape[1], n_class, buf.data_ptr(), buf.data_ptr() + 4 * n,
                                buf.data_ptr() + 4 * (n + B), B, T, stream()))
    return buf[n + B:n + 2 * B].view(torch.float32)


def attn_confidence(logits, ids, eos):
    """A greedy attention decoder's score (utils.confidence.attn_score): logits (B, steps, n_class) float32, ids (B, steps) int32
    -> one int32 buffer (2 B): the bits of the float32 scores (`buf[:B].view(torch.float32)`), then the terms."""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and logits.is_contiguous()):
        raise _abi.DpmnError("attn_confidence: contiguous float32 CUDA logits (B, steps, n_class) expected; there is no CPU fallback")
    B, steps, n_class = logits.shape
    if tuple(ids.shape) != (B, steps) or ids.device != logits.device:
        raise _abi.DpmnError("attn_confidence: ids (B, steps) on the logits' device expected")
    buf = torch.empty(2 * B, dtype=torch.int32, device=logits.device)
    check(lib.dpmn_attn_conf_f32(dptr(logits), _i32(ids, "attn_confidence"), int(eos), buf.data_ptr(), buf.data_ptr() + 4 * B,
                                 B, steps, n_class, stream()))
    return buf


def turn180(x):
    """x (B, C, H, W) float32 turned by 180 degrees in every plane: bitwise x.flip(2, 3), as a new contiguous tensor."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
        raise _abi.DpmnError("turn180: a non-empty float32 CUDA tensor (B, C, H, W) expected; there is no CPU fallback")
    x = x.contiguous()
    y = torch.empty_like(x)
    B, Cc, H, W = x.shape
    check(lib.dpmn_turn180_f32(dptr(x), dptr(y), B, Cc, H, W, stream()))
    return y


# ------------------------------------------------------------------------------ one read per tiled line (csrc/line_read.hip)
class LineTable:
    """The lines of a ragged batch of line posteriors (utils/line_read.py): `host`, an int32 (B, 2) array of [first row of line_lp, L]
    per image -- the lines back to back from row 0, every L >= 1 -- `frames` = the sum of the L and `max_L`.  Iterating gives
    (first row, L) tuples.  The table is uploaded once per device and kept for the launches that read it."""

    def __init__(self, table):
        import numpy as np
        host = np.ascontiguousarray(np.asarray(table, np.int64).reshape(-1, 2))
        if not len(host) or (host[:, 1] < 1).any() or host[0, 0] != 0 or (host[1:, 0] != np.cumsum(host[:-1, 1])).any():
            raise _abi.DpmnError("LineTable: (first row, L >= 1) per line expected, the lines back to back from row 0")
        if host.sum(1).max() > 2 ** 31 - 1:
            raise _abi.DpmnError("LineTable: the batch has more rows than an int32 counts")
        self.host = host.astype(np.int32)
        self.frames, self.max_L = int(host[:, 1].sum()), int(host[:, 1].max())
        self._dev = {}

    def __len__(self):
        return len(self.host)

    def __iter__(self):
        return iter([(int(f), int(n)) for f, n in self.host])

    def __array__(self, dtype=None, copy=None):
        return self.host if dtype is None else self.host.astype(dtype)

    def device_ptr(self, device):
        """The device pointer of the table on `device` (uploaded on first use)."""
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            self._dev[key] = _upload(torch.device("cuda", key), self.host)
        return self._dev[key][1]


def _line_lp(line_lp, lines, what):
    """The checks the two ops on line posteriors share -> (the LineTable, n_class)."""
    if not isinstance(lines, LineTable):
        lines = LineTable(lines)
    if not (torch.is_tensor(line_lp) and line_lp.is_cuda and line_lp.dtype == torch.float32 and line_lp.dim() == 2
            and line_lp.is_contiguous() and line_lp.shape[0] == lines.frames and line_lp.shape[1] >= 1):
        raise _abi.DpmnError("%s: contiguous float32 CUDA line posteriors (%d, n_class) expected, one row per frame of the table; there "
                             "is no CPU fallback" % (what, lines.frames))
    return lines, line_lp.shape[1]


def line_stitch(rows, T, n_class, plan, lr_w):
    """The frame posteriors of the windows of a tile plan blended into one posterior per LINE frame (utils.line_read.stitch_lp_np):
    rows (windows * T, ld >= n_class) logits, row w*T + t (NativeCRNN.window_rows' layout; the padding columns are not read), plan the
    windows' (image, x0) (utils/tile.py), lr_w the window width in columns -> (line_lp, lines): the float32 (sum L_b, n_class)
    log-posteriors of every image's line, back to back, and their LineTable."""
    import numpy as np
    from .utils.line_read import covered_lines
    T, n_class, lr_w = int(T), int(n_class), int(lr_w)
    if not (torch.is_tensor(rows) and rows.is_cuda):
        raise _abi.DpmnError("line_stitch: the windows' logits are blended on the GPU (got a %s tensor); there is no CPU fallback"
                             % (rows.device if torch.is_tensor(rows) else type(rows).__name__))
    if rows.dim() != 2 or T < 2 or lr_w < 2 or n_class < 1 or not len(plan) or rows.shape[0] != len(plan) * T or rows.shape[1] < n_class:
        raise _abi.DpmnError("line_stitch: logits rows (windows * T, >= n_class) with T >= 2 and a plan of as many windows expected, got "
                             "%s, T %d, %d classes, %d windows" % (tuple(rows.shape), T, n_class, len(plan)))
    try:
        per_line = covered_lines(plan, lr_w)
    except ValueError as e:
        raise _abi.DpmnError("line_stitch: %s" % e) from e
    L = [(w_line * (T - 1)) // lr_w + 1 for _, _, w_line in per_line]
    lines = LineTable(np.stack([np.concatenate(([0], np.cumsum(L[:-1]))), L], 1))
    d, d_lines, d_wins, d_x0 = _upload(rows.device, lines.host, np.array([l[:2] for l in per_line], np.int32),
                                       np.ascontiguousarray(np.asarray(plan, np.int32).reshape(-1, 2)[:, 1]))
    lines._dev[d.device.index] = (d, d_lines)
    line_lp = torch.empty(lines.frames, n_class, device=rows.device)
    check(lib.dpmn_line_stitch_f32(dptr(rows), rows.shape[1], n_class, T, lr_w, d_lines, d_wins, d_x0, len(lines), lines.max_L,
                                   dptr(line_lp), stream()))
    return line_lp, lines


def line_greedy(line_lp, lines, extra=0):
    """The greedy CTC decode of every line (utils.line_read.greedy_np): line_lp (N = sum L_b, n_class), lines its LineTable (or a host
    (B, 2) table) -> one int32 buffer (3 N + B + extra): cls (N), start (N), end (N), length (B).  A line's entries stand at its first
    row: the collapsed classes, then per kept symbol the first and the last line frame of its arg-max run, zero behind the length.
    Returned as (buffer, cls, start, end, length) views, so that the host reads everything with one copy; extra as for ctc_greedy."""
    lines, n_class = _line_lp(line_lp, lines, "line_greedy")
    N, B = lines.frames, len(lines)
    buf = torch.empty(3 * N + B + int(extra), dtype=torch.int32, device=line_lp.device)
    p = buf.data_ptr()
    check(lib.dpmn_line_greedy_i32(dptr(line_lp), n_class, lines.device_ptr(line_lp.device), B, lines.max_L, p, p + 4 * N, p + 8 * N,
                                   p + 12 * N, stream()))
    return buf, buf[:N], buf[N:2 * N], buf[2 * N:3 * N], buf[3 * N:3 * N + B]


def line_ctc_confidence(line_lp, lines, buf):
    """The CTC log-likelihood of every line's own greedy string (utils.line_read.line_score_np): buf = line_greedy's buffer made with
    extra >= B.  The float32 score bits go behind the lengths, `buf[3 N + B:3 N + 2 B].view(torch.float32)` (returned), as
    ctc_confidence writes them."""
    lines, n_class = _line_lp(line_lp, lines, "line_ctc_confidence")
    N, B = lines.frames, len(lines)
    if not (torch.is_tensor(buf) and buf.device == line_lp.device and buf.dtype == torch.int32 and buf.is_contiguous()
            and buf.dim() == 1 and buf.numel() >= 3 * N + 2 * B):
        raise _abi.DpmnError("line_ctc_confidence: buf must be ops.line_greedy's int32 buffer with extra >= B")
    p = buf.data_ptr()
    check(lib.dpmn_line_ctc_f32(dptr(line_lp), n_class, lines.device_ptr(line_lp.device), p, p + 12 * N, p + 4 * (3 * N + B), B,
                                lines.max_L, stream()))
    return buf[3 * N + B:3 * N + 2 * B].view(torch.float32)


# ------------------------------------------------------------------------------ a tiled line as lexicon words (csrc/line_words.hip)
LINE_WORDS_BLOCK = lib.dpmn_line_words_block()      # the trie nodes one block of the frame-per-launch arm covers
LINE_WORDS_ARMS = ("step", "lds")                   # dpmn_line_words_f64's arm 0 / 1


def line_words_lds_nodes(device):
    """The most trie nodes the single-launch arm holds in the LDS of `device`."""
    with torch.cuda.device(device):
        return int(lib.dpmn_line_words_lds_nodes())


def line_words_arm(nodes, device):
    """The arm ops.line_words takes for a trie of `nodes` nodes on `device`: 'lds' (one launch per call, the state in LDS) while the
    trie fits the device's LDS, else 'step' (one launch per frame).  Measured (profiles/line_words_bench.json): the single launch
    is the faster one wherever it can run."""
    return "lds" if int(nodes) <= line_words_lds_nodes(device) else "step"


def line_words_records(line_lp, lines, lex, penalty=0.0, out=None, arm=None):
    """The launches of line_words -> one int32 buffer (3 N + 4 B): per line frame the word of E[t], its start and whether G[t] was
    entered from E[t-1], then per line the fp64 bits of G[L-1] and E[L-1] (utils.line_words.decode_records reads them).  out: write
    into this int32 tensor of 3 N + 4 B elements instead (line_greedy's `extra`); arm: None (line_words_arm's), 'step' or 'lds'."""
    import math
    if not isinstance(lex, Lexicon):
        raise _abi.DpmnError("line_words: lex must be an ops.Lexicon")
    if not isinstance(lines, LineTable):
        lines = LineTable(lines)
    if not (torch.is_tensor(line_lp) and line_lp.is_cuda and line_lp.dtype == torch.float32 and line_lp.dim() == 2
            and line_lp.shape[0] == lines.frames and line_lp.shape[1] >= 1 and line_lp.stride(1) == 1
            and line_lp.stride(0) >= line_lp.shape[1]):
        raise _abi.DpmnError("line_words: float32 CUDA line posteriors (%d, n_class) with unit column stride expected, one row per frame "
                             "of the table; there is no CPU fallback" % lines.frames)
    n_class, N, B = line_lp.shape[1], lines.frames, len(lines)
    if lex.max_class >= n_class:
        raise _abi.DpmnError("line_words: the lexicon holds class %d, the line has %d classes" % (lex.max_class, n_class))
    if not math.isfinite(float(penalty)):
        raise _abi.DpmnError("line_words: the penalty must be finite, got %r" % (penalty,))
    trie = lex.device_trie(line_lp.device)
    nodes = trie.numel() // 4
    arm = line_words_arm(nodes, line_lp.device) if arm is None else arm
    if arm not in LINE_WORDS_ARMS:
        raise _abi.DpmnError("line_words: arm is None, 'step' or 'lds', got %r" % (arm,))
    if out is None:
        out = torch.empty(3 * N + 4 * B, dtype=torch.int32, device=line_lp.device)
    elif not (torch.is_tensor(out) and out.device == line_lp.device and out.dtype == torch.int32 and out.is_contiguous()
              and out.numel() == 3 * N + 4 * B):
        raise _abi.DpmnError("line_words: out must be a contiguous int32 tensor of 3 N + 4 B elements on %s" % line_lp.device)
    ws = lex.workspace(line_lp.device, lib.dpmn_line_words_workspace_bytes(B, N, nodes)) if arm == "step" else None
    p = out.data_ptr()
    with torch.cuda.device(line_lp.device):
        check(lib.dpmn_line_words_f64(line_lp.data_ptr(), line_lp.stride(0), n_class, lines.device_ptr(line_lp.device), B, lines.max_L, N,
                                      trie.data_ptr(), nodes, float(penalty), LINE_WORDS_ARMS.index(arm), p, p + 4 * N, p + 8 * N,
                                      p + 12 * N, ws.data_ptr() if ws is not None else None, stream()))
    return out


def line_words_decode(h, lines):
    """The host half: h = line_words_records' buffer as a NumPy int32 array -> per line (word indices, spans, score)."""
    from .utils.line_words import decode_records
    N, B = lines.frames, len(lines)
    fin = h[3 * N:3 * N + 4 * B].view("float64").reshape(B, 2)
    return [decode_records(L, fin[b], h[f0:f0 + L], h[N + f0:N + f0 + L], h[2 * N + f0:2 * N + f0 + L])
            for b, (f0, L) in enumerate(lines)]


def line_words(line_lp, lines, lex, penalty=0.0, arm=None):
    """Every line read as a sequence of lexicon words (utils.line_words.line_words_np: the one-pass Viterbi over "blank gap, word,
    blank gap, ..."): line_lp (N = sum L_b, n_class) float32 log-posteriors (ops.line_stitch's; rows may be a column slice of a
    wider buffer, the columns behind n_class are not read), lines its LineTable (or a host (B, 2) table), lex an ops.Lexicon,
    penalty a finite float added once per word -> per line (word indices, [(first, last)] spans, score), the score a float64 with
    the restatement's bits.  ONE device-to-host copy.  arm: line_words_records'."""
    if not isinstance(lines, LineTable):
        lines = LineTable(lines)
    out = line_words_records(line_lp, lines, lex, penalty, arm=arm)
    return line_words_decode(out.cpu().numpy(), lines)


# ------------------------------------------------------------------------------ native ASTER recogniser (csrc/aster.hip)
def aster_prep(img, stn_h=32, stn_w=64):
    """parse_aster_data + the STN head's bilinear (align_corners=True) resize for a batch: (B, >=3, H, W) in [0, 1] ->
    (normalised NCHW (B, 3, H, W), NHWC (B, stn_h, stn_w, 4) with channel 3 zero)."""
    B, Cc, H, W = img.shape
    if Cc < 3:
        raise _abi.DpmnError("aster_prep: channels 0..2 (RGB) are read, got %d channels" % Cc)
    v, ptr, stride = _nchw_view(img)
    norm = torch.empty(B, 3, H, W, device=img.device)
    stn = torch.empty(B, stn_h, stn_w, 4, device=img.device)
    check(lib.dpmn_aster_prep_f32(ptr, stride, dptr(norm), dptr(stn), B, H, W, stn_h, stn_w, stream()))
    return norm, stn


def subsample_nhwc(x, sy, sx):
    """x[:, ::sy, ::sx, :] of an NHWC tensor as a contiguous tensor (the gather in front of a 1 x 1 conv with stride (sy, sx))."""
    B, H, W, Cc = x.shape
    y = torch.empty(B, (H - 1) // sy + 1, (W - 1) // sx + 1, Cc, device=x.device)
    check(lib.dpmn_subsample_nhwc_f32(dptr(x), dptr(y), B, H, W, Cc, sy, sx, stream()))
    return y


def aster_dec_weights(tensors):
    """dict name -> tensor (the fields of dpmn_aster_dec_weights) -> a filled _abi.AsterDecWeights; the caller keeps the tensors."""
    w = _abi.AsterDecWeights()
    for n in _abi.AsterDecWeights.NAMES:
        setattr(w, n, dptr(tensors[n]))
    return w


def _i32(t, what):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise _abi.DpmnError("dpmn_amd: %s expects a contiguous int32 CUDA tensor" % what)
    return t.data_ptr()


def aster_decode_step(weights, feats, xproj, row_img, state, y_prev, n_class):
    """One teacher-forced decoder step for R rows (row r attends to image row_img[r]) -> (logits (R, n_class), new state
    (R, 512), alpha (R, T))."""
    import ctypes as _C
    R, T = state.shape[0], feats.shape[1]
    if tuple(feats.shape) != tuple(xproj.shape) or feats.shape[2] != 512 or tuple(state.shape) != (R, 512) or row_img.numel() != R or y_prev.numel() != R:
        raise _abi.DpmnError("aster_decode_step: feats / xproj (B, T, 512), state (R, 512), row_img / y_prev (R) expected")
    dev = state.device
    sproj, ctx, out = torch.empty(R, 512, device=dev), torch.empty(R, 512, device=dev), torch.empty(R, 512, device=dev)
    alpha, logits = torch.empty(R, T, device=dev), torch.empty(R, n_class, device=dev)
    check(lib.dpmn_aster_decode_step_f32(_C.byref(weights), dptr(feats), dptr(xproj), _i32(row_img, "aster_decode_step"), dptr(state),
                                         _i32(y_prev, "aster_decode_step"), dptr(sproj), dptr(ctx), dptr(alpha), dptr(out), dptr(logits),
                                         R, T, n_class, stream()))
    return logits, out, alpha


def aster_beam(weights, feats, xproj, beam, n_class, eos, steps):
    """Beam search on the current stream -> ONE int32 buffer (3, steps, B * beam): emitted symbols, predecessor rows and the bits
    of the float32 sequence scores of every step (one device-to-host copy serves the host backtracking)."""
    import ctypes as _C
    B, T, D = feats.shape
    if tuple(xproj.shape) != (B, T, D) or D != 512:
        raise _abi.DpmnError("aster_beam: feats and xproj (B, T, 512) expected")
    R = B * beam
    nb = lib.dpmn_aster_beam_workspace_bytes(B, beam)
    ws = torch.empty(nb // 4, device=feats.device)
    buf = torch.empty(3, steps, R, dtype=torch.int32, device=feats.device)
    n = 4 * steps * R
    check(lib.dpmn_aster_beam_f32(_C.byref(weights), dptr(feats), dptr(xproj), dptr(ws), nb, buf.data_ptr(), buf.data_ptr() + n,
                                  buf.data_ptr() + 2 * n, B, T, beam, n_class, eos, steps, stream()))
    return buf


# ------------------------------------------------------------------------------ native MORAN recogniser (csrc/moran.hip)
def moran_prep(img, out_h=32, out_w=100):
    """parse_moran_data (base.py:396-402) for a batch: (B, >=3, H, W) in [0, 1] -> (luma plane (B, 1, out_h, out_w), the same as NHWC
    (B, out_h, out_w, 4) with channels 1..3 zero)."""
    return _gray_prep("moran_prep", img, out_h, out_w, True)


def moran_rectify(omap, plane, grid_x, grid_y, acc=None):
    """One pass of MORN behind its offset head: omap (B, Hm, Wm), plane (B, 1, H, W), acc = the running offsets (B, H, W) or None on
    the first pass -> (new accumulated offsets, rectified plane (B, 1, H, W), rectified NHWC (B, H, W, 4))."""
    B, _, H, W = plane.shape
    if omap.dim() != 3 or omap.shape[0] != B or grid_x.numel() != W or grid_y.numel() != H or (acc is not None and tuple(acc.shape) != (B, H, W)):
        raise _abi.DpmnError("moran_rectify: omap (B, Hm, Wm), plane (B, 1, H, W), grid_x (W), grid_y (H), acc (B, H, W) expected")
    new = torch.empty(B, H, W, device=plane.device)
    rect = torch.empty(B, 1, H, W, device=plane.device)
    rect4 = torch.empty(B, H, W, 4, device=plane.device)
    check(lib.dpmn_moran_rectify_f32(dptr(omap), dptr(plane), dptr(grid_x), dptr(grid_y), dptr(acc, True), dptr(new), dptr(rect),
                                     dptr(rect4), B, H, W, omap.shape[1], omap.shape[2], stream()))
    return new, rect, rect4


def moran_split(x, sy, sx):
    """x (B, H, W, 2 C) -> (x[:, ::sy, ::sx, :C], x[:, ::sy, ::sx, C:]) as contiguous tensors."""
    B, H, W, C2 = x.shape
    Cc = C2 // 2
    y1 = torch.empty(B, (H - 1) // sy + 1, (W - 1) // sx + 1, Cc, device=x.device)
    y2 = torch.empty_like(y1)
    check(lib.dpmn_moran_split_nhwc_f32(dptr(x), dptr(y1), dptr(y2), B, H, W, Cc, sy, sx, stream()))
    return y1, y2


def moran_dec_weights(tensors):
    """dict name -> tensor (the fields of dpmn_moran_dec_weights) -> a filled _abi.MoranDecWeights; the caller keeps the tensors."""
    w = _abi.MoranDecWeights()
    for n in _abi.MoranDecWeights.NAMES:
        setattr(w, n, dptr(tensors[n]))
    return w


def moran_decode(weights, feats, fproj, steps, n_class):
    """The greedy L2R decoder on the current stream: feats / fproj (B, T, 256) -> (logits (B, steps, n_class), ids (B, steps) int32)."""
    import ctypes as _C
    B, T, D = feats.shape
    if tuple(fproj.shape) != (B, T, D) or D != 256:
        raise _abi.DpmnError("moran_decode: feats and fproj (B, T, 256) expected")
    logits = torch.empty(B, steps, n_class, device=feats.device)
    ids = torch.empty(B, steps, dtype=torch.int32, device=feats.device)
    check(lib.dpmn_moran_decode_f32(_C.byref(weights), dptr(feats), dptr(fproj), dptr(logits), ids.data_ptr(), B, T, steps, n_class, stream()))
    return logits, ids
