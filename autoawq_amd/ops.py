"""Host-side operators: torch tensors in, torch tensors out, work done by libawq_hip.so.

PyTorch is plumbing here (device memory, current stream); every computation is a hand-written
gfx950 kernel reached through the C ABI of include/awq_hip.h.
"""
import ctypes
import math

import torch

from . import _lib

# kernel-selection flags (mirror include/awq_hip.h)
KERNEL_AUTO, KERNEL_NAIVE, KERNEL_VALU, KERNEL_MFMA_GEMV, KERNEL_TILED, KERNEL_REGB, KERNEL_SKINNY = 0, 1, 2, 3, 4, 5, 6
FLAG_TWO_PASS = 1 << 16
FLAG_NO_NT = 1 << 17


def gemm_flags(kernel=0, nlog=0, splitk=0, two_pass=False, no_nt=False, waves=0, unit=0):
    """nlog: VALU -> log2 column lanes (2..4); MFMA_GEMV -> packed words per lane (2|4);
    waves / unit: MFMA_GEMV waves per block and 16-row sets per wave iteration."""
    f = (kernel & 0xF) | ((nlog & 0xF) << 4) | ((splitk & 0xFF) << 8) | ((waves & 0xF) << 24) | ((unit & 0xF) << 20)
    if two_pass:
        f |= FLAG_TWO_PASS
    if no_nt:
        f |= FLAG_NO_NT
    return f


def _require_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.AwqHipError(
                "autoawq_amd kernels run on a HIP device (MI355X); got a tensor on "
                f"'{t.device}'. There is no CPU fallback.")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


_workspaces = {}   # (device index, stream handle) -> _Workspace
_retired = []      # outgrown workspaces: a hipGraph captured earlier may still hold their pointers
_retired_raw = []  # the same for the MoE / attention scratch tensors
_CHECK_EVERY = 64  # calls between two asynchronous read-backs of a workspace's error word


class _Workspace:
    """One split-K workspace (control words + exchange + scratch) of one stream, with an asynchronous
    watch on its error word: the kernels never hang -- a reducer that gives up waiting raises word 0
    and uses what is there (csrc/gemv_mfma.hip) -- so somebody has to look at that word.  Every
    `_CHECK_EVERY` calls a 4-byte device->pinned-host copy is queued behind the work; the next call
    that finds the copy complete inspects it, re-initialises the workspace and raises."""

    def __init__(self, device, nbytes):
        # (created OUTSIDE inference mode whatever the caller's mode is: a workspace first needed inside `torch.inference_mode()` --
        #  the fused model's forward -- would otherwise hold inference tensors, and the read-back below, issued later from an
        #  ordinary context, would raise "Inplace update to inference tensor outside InferenceMode")
        with torch.inference_mode(False):
            self.buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.calls = 0
        self.event = None
        self.init()

    def init(self):
        _lib.check(_lib.lib().awq_gemm_workspace_init(_ptr(self.buf), self.buf.numel(), _stream()), "awq_gemm_workspace_init")

    def numel(self):
        return self.buf.numel()

    def poll(self):
        """non-blocking: look at a finished read-back, start a new one now and then (never while capturing)"""
        if torch.cuda.is_current_stream_capturing():
            return
        if self.event is not None and self.event.query():
            self.event = None
            if int(self.host[0]) != 0:
                self.host.zero_()
                self.init()
                raise _lib.AwqHipError("a split-K reducer gave up waiting for its partial sums on this workspace "
                                       "(control word != 0): results since the last check are unreliable; the "
                                       "workspace has been re-initialised")
        self.calls += 1
        if self.event is None and self.calls % _CHECK_EVERY == 0:
            self.host.copy_(self.buf[:4].view(torch.int32), non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()


def workspace(device, nbytes):
    """Split-K workspace, one per (device, stream), grown on demand and prepared once by
    awq_gemm_workspace_init (control words zero, exchange region = all-ones sentinel); every kernel
    that uses it restores that state.  A workspace that has to grow is RETIRED, not freed: a hipGraph
    captured earlier on the stream keeps replaying into the old buffer (`release_workspaces()` drops
    them all once no such graph is alive)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _retired.append(ws)
        ws = _Workspace(device, nbytes)
        _workspaces[key] = ws
    ws.poll()
    return ws.buf


def _current_workspace(device):
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    ws = _workspaces.get(key)
    return None if ws is None else ws.buf


def check_workspaces():
    """Blocking form of the error watch: synchronises and raises if any workspace's error word is set
    (after re-initialising it)."""
    torch.cuda.synchronize()
    bad = []
    for key, ws in list(_workspaces.items()) + [(None, w) for w in _retired]:
        if int(ws.buf[:4].view(torch.int32).item()) != 0:
            bad.append(key)
            with torch.cuda.device(ws.buf.device):
                ws.init()
    for d in (_moe_workspaces,):
        for key, buf in d.items():
            if int(buf[:4].view(torch.int32).item()) != 0:
                bad.append(key)
                with torch.cuda.device(buf.device):
                    _lib.check(_lib.lib().awq_gemm_workspace_init(_ptr(buf), buf.numel(), _stream()), "awq_gemm_workspace_init")
    torch.cuda.synchronize()
    if bad:
        raise _lib.AwqHipError(f"split-K error word set on workspace(s) {bad}: a reducer gave up waiting; re-initialised")


def release_workspaces():
    """Free every workspace (current and retired).  Only when no captured hipGraph that used them is
    going to be replayed again."""
    torch.cuda.synchronize()
    _workspaces.clear()
    _moe_workspaces.clear()
    _attn_workspaces.clear()
    _expert_workspaces.clear()
    del _retired[:]
    del _retired_raw[:]


def workspace_is_clean(device):
    """True when the workspace is back in its initial state: error flag / control words zero and the
    split-K exchange region (first half after the control words) all-ones again."""
    ws = _current_workspace(device)
    if ws is None:
        return True
    half = ((ws.numel() - 16384) // 2) & ~255
    return (not bool(ws[:16384].any().item())) and bool((ws[16384:16384 + half] == 0xFF).all().item())


def unpack_int4(q):
    """[rows, words] int32 -> [rows, 8*words] uint8 logical nibbles (awq_unpack_int4)."""
    _require_gpu(q)
    q = q.contiguous()
    out = torch.empty((q.shape[0], q.shape[1] * 8), dtype=torch.uint8, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().awq_unpack_int4(_ptr(q), _ptr(out), q.shape[0], q.shape[1], _stream()), "awq_unpack_int4")
    return out


def dequantize_weights(qweight, scales, qzeros):
    """GEMM-layout buffers -> fp16 W [K, N] (awq_dequantize_weights)."""
    _require_gpu(qweight, scales, qzeros)
    qweight, scales, qzeros = qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    K, N = qweight.shape[0], qweight.shape[1] * 8
    G = qzeros.shape[0]
    if G == 0 or K % G:
        raise _lib.AwqHipError("dequantize_weights: qzeros rows do not divide in_features")
    out = torch.empty((K, N), dtype=torch.float16, device=qweight.device)
    with torch.cuda.device(qweight.device):
        _lib.check(_lib.lib().awq_dequantize_weights(_ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(out), K, N,
                                                     K // G, _stream()), "awq_dequantize_weights")
    return out


X_GATED_SILU = 1 << 18  # AWQ_GEMM_FLAG_X_GATED_SILU


def _gemm_operands(name, x2d, qweight, scales, qzeros, gated=False):
    """GEMM layout: the operands of the wrapper `name`, checked (on a HIP device, fp16 activations, matching shapes) and contiguous,
    a fresh output [M, N] and the sizes the library takes (gated: x2d is [M, 2K] = [gate | up]):
    (x2d, qweight, scales, qzeros, y, M, K, N, group_size)"""
    _require_gpu(x2d, qweight, scales, qzeros)
    if x2d.dtype != torch.float16:
        raise _lib.AwqHipError(f"{name} expects fp16 activations")
    x2d, qweight, scales, qzeros = x2d.contiguous(), qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    M, K = x2d.shape
    if gated:
        K //= 2
    N, G = qweight.shape[1] * 8, qzeros.shape[0]
    if qweight.shape[0] != K or G == 0 or K % G:
        raise _lib.AwqHipError(f"{name}: shape mismatch x{tuple(x2d.shape)} qweight{tuple(qweight.shape)} qzeros{tuple(qzeros.shape)}")
    y = torch.empty((M, N), dtype=torch.float16, device=x2d.device)
    return x2d, qweight, scales, qzeros, y, M, K, N, K // G


def _gemm_workspace(device, M, K, N, group_size, optional=False):
    """(pointer, bytes) of the current stream's split-K workspace, grown to what this call needs (optional: none where it needs none)"""
    need = _lib.lib().awq_gemm_workspace_bytes(M, K, N, group_size)
    ws = workspace(device, need) if need or not optional else None
    return _ptr(ws), ws.numel() if ws is not None else 0


def gemm_forward(x2d, qweight, scales, qzeros, bias=None, flags=0):
    """y [M, N] fp16 = x2d [M, K] fp16 @ dequant(GEMM-layout buffers) (+ bias) (awq_gemm_forward).
    With flags | X_GATED_SILU, x2d is [M, 2K] = [gate | up] and the kernel applies silu(gate) * up
    while staging (M <= 16)."""
    _require_gpu(bias)
    x2d, qweight, scales, qzeros, y, M, K, N, g = _gemm_operands("gemm_forward", x2d, qweight, scales, qzeros, flags & X_GATED_SILU)
    if M == 0:
        return y
    with torch.cuda.device(x2d.device):
        rc = _lib.lib().awq_gemm_forward(_ptr(x2d), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(bias), _ptr(y), M, K, N, g,
                                         *_gemm_workspace(x2d.device, M, K, N, g, optional=True), flags, _stream())
    _lib.check(rc, "awq_gemm_forward")
    return y


def grouped_gemm_prefill(x_sorted, qweight, scales, qzeros, seg_offsets, flags=0):
    """MoE prefill (awq_grouped_gemm_prefill): x_sorted [P, K] fp16 = the (token, expert) pairs' rows sorted by expert,
    seg_offsets [E + 1] int32 on the device, qweight [E, K, N/8] / scales [E, K/g, N] / qzeros [E, K/g, N/8] the stacked
    GEMM-layout experts -> y [P, N].  No routing data is read back: capturable."""
    x_sorted, qweight, scales, qzeros, seg, P, E, K, N, g = _grouped_prefill_operands(
        "grouped_gemm_prefill", x_sorted, qweight, scales, qzeros, seg_offsets)
    y = torch.empty((P, N), dtype=torch.float16, device=x_sorted.device)
    with torch.cuda.device(x_sorted.device):
        rc = _lib.lib().awq_grouped_gemm_prefill(_ptr(x_sorted), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(y), _ptr(seg),
                                                 P, E, K, N, g, flags, _stream())
    _lib.check(rc, "awq_grouped_gemm_prefill")
    return y


GROUPED_PREFILL_GATHER_X, GROUPED_PREFILL_SCATTER_Y = 1 << 19, 1 << 20


def moe_sort_pairs(topk_ids, num_experts):
    """(order [P] int32, seg_offsets [E + 1] int32): the pairs of topk_ids [T, topk] grouped by expert as an index list, one
    launch (awq_moe_sort_pairs) == torch.argsort(topk_ids.flatten(), stable=True) + the experts' row ranges."""
    _require_gpu(topk_ids)
    ids = topk_ids.contiguous().view(-1)
    if ids.dtype != torch.int32:
        raise _lib.AwqHipError("moe_sort_pairs expects int32 topk_ids")
    order = torch.empty_like(ids)
    seg = torch.empty((num_experts + 1,), dtype=torch.int32, device=ids.device)
    with torch.cuda.device(ids.device):
        _lib.check(_lib.lib().awq_moe_sort_pairs(_ptr(ids), _ptr(order), _ptr(seg), ids.numel(), num_experts, _stream()),
                   "awq_moe_sort_pairs")
    return order, seg


def _grouped_prefill_operands(name, x, qweight, scales, qzeros, seg_offsets, row_map=None):
    """The grouped prefill GEMM's operands, checked and contiguous, and its sizes (P: the row map's length, else x's rows):
    (x, qweight, scales, qzeros, seg_offsets, P, E, K, N, group_size)"""
    _require_gpu(x, qweight, scales, qzeros, seg_offsets, row_map)
    if x.dtype != torch.float16 or seg_offsets.dtype != torch.int32 or (row_map is not None and row_map.dtype != torch.int32):
        raise _lib.AwqHipError(f"{name} expects fp16 activations and int32 offsets / row map")
    x, qweight, scales, qzeros = x.contiguous(), qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    P, K = x.shape[0] if row_map is None else row_map.numel(), x.shape[1]
    E, N, G = qweight.shape[0], qweight.shape[2] * 8, qzeros.shape[1]
    if qweight.shape[1] != K or scales.shape != (E, G, N) or qzeros.shape != (E, G, N // 8) or seg_offsets.numel() != E + 1 or K % G:
        raise _lib.AwqHipError(f"{name}: shape mismatch x{tuple(x.shape)} qweight{tuple(qweight.shape)} "
                               f"scales{tuple(scales.shape)} qzeros{tuple(qzeros.shape)} seg{tuple(seg_offsets.shape)}")
    return x, qweight, scales, qzeros, seg_offsets.contiguous(), P, E, K, N, K // G


def grouped_gemm_prefill_ex(x, qweight, scales, qzeros, seg_offsets, row_map, x_div=1, gather=False, scatter=False,
                            pair_weights=None, flags=0, zero_init=False):
    """awq_grouped_gemm_prefill_ex: the grouped prefill GEMM with the sort kept as an index list.  gather: x [T, K] holds the
    tokens, sorted row r reads row row_map[r] / x_div; else x [P, K] is sorted.  scatter: y row row_map[r] (pair order) instead
    of r; pair_weights [P] fp32 by pair index multiply the fp32 product before its one rounding."""
    _require_gpu(pair_weights)
    x, qweight, scales, qzeros, seg, P, E, K, N, g = _grouped_prefill_operands(
        "grouped_gemm_prefill_ex", x, qweight, scales, qzeros, seg_offsets, row_map)
    if (gather and x.shape[0] * x_div < P) or (not gather and x.shape[0] != P):
        raise _lib.AwqHipError(f"grouped_gemm_prefill_ex: x{tuple(x.shape)} does not cover {P} pairs (x_div {x_div})")
    w = pair_weights.contiguous().float().view(-1) if pair_weights is not None else None
    if w is not None and w.numel() != P:
        raise _lib.AwqHipError("grouped_gemm_prefill_ex: one routing weight per pair")
    y = (torch.zeros if zero_init else torch.empty)((P, N), dtype=torch.float16, device=x.device)
    f = flags | (GROUPED_PREFILL_GATHER_X if gather else 0) | (GROUPED_PREFILL_SCATTER_Y if scatter else 0)
    with torch.cuda.device(x.device):
        rc = _lib.lib().awq_grouped_gemm_prefill_ex(_ptr(x), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(y), _ptr(seg),
                                                    _ptr(row_map.contiguous()), _ptr(w), P, x_div, E, K, N, g, f, _stream())
    _lib.check(rc, "awq_grouped_gemm_prefill_ex")
    return y


def _gemv_operands(name, x2d, qweight, scales, qzeros, halve=False):
    """GEMV layout: the operands of the wrapper `name`, checked (on a HIP device, fp16 activations, matching shapes) and contiguous,
    a fresh output [M, N] (halve: [M, N / 2]) and the sizes the library takes: (x2d, qweight, scales, qzeros, y, M, K, N, ZW)"""
    _require_gpu(x2d, qweight, scales, qzeros)
    if x2d.dtype != torch.float16:
        raise _lib.AwqHipError(f"{name} expects fp16 activations")
    x2d, qweight, scales, qzeros = x2d.contiguous(), qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    M, K = x2d.shape
    N, ZW = qweight.shape[0], qzeros.shape[1]
    if qweight.shape[1] * 8 != K or scales.shape != (N, ZW * 8):
        raise _lib.AwqHipError(f"{name}: shape mismatch x{tuple(x2d.shape)} qweight{tuple(qweight.shape)} "
                               f"qzeros{tuple(qzeros.shape)} scales{tuple(scales.shape)}")
    y = torch.empty((M, N // 2 if halve else N), dtype=torch.float16, device=x2d.device)
    return x2d, qweight, scales, qzeros, y, M, K, N, ZW


def _forward_rows(fn, x2d, qweight, scales, qzeros, y, chunk, *sizes_flags):
    """awq_gemv_forward / awq_gemv_fast_forward (`fn`) on `chunk` rows of x2d at a time; the first code that is not 0, else 0"""
    M = x2d.shape[0]
    with torch.cuda.device(x2d.device):
        for m0 in range(0, M, chunk):
            m1 = min(M, m0 + chunk)
            rc = fn(_ptr(x2d[m0:m1]), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(y[m0:m1]), m1 - m0, *sizes_flags, _stream())
            if rc:
                return rc
    return 0


def _decode_chunk(lds_bytes):
    """Rows per call of the 16-row decode kernels: at most 16, halved while the kernel's LDS (lds_bytes(rows)) exceeds 160 KiB"""
    chunk = 16
    while chunk > 1 and lds_bytes(chunk) > 160 * 1024:
        chunk //= 2
    return chunk


def gemv_forward(x2d, qweight, scales, qzeros, group_size, flags=0):
    """GEMV layout (qweight [N, K/8], qzeros [N, ZW], scales [N, 8*ZW]): y [M, N] fp16 = x2d @ W^T
    (awq_gemv_forward).  M is processed in chunks that fit the kernel (<= 16 rows and the LDS)."""
    x2d, qweight, scales, qzeros, y, M, K, N, ZW = _gemv_operands("gemv_forward", x2d, qweight, scales, qzeros)
    if M == 0:
        return y
    L = _lib.lib()
    kern = flags & 0xF
    # ONE call: PREFILL (explicit only: the register-decoded MFMA GEMM, any M; latency-bound below ~2000 rows, include/awq_hip.h) and
    # the batched kernel (csrc/gemv_batch.hip: launches of <= 128 rows inside the library), named or the library's AUTO choice
    one_call = kern in (GEMV_KERNEL_PREFILL, GEMV_KERNEL_BATCH) or (kern == 0 and gemv_auto_kernel(M, K, N, group_size) == GEMV_KERNEL_BATCH)
    chunk = M if one_call else _decode_chunk(lambda rows: L.awq_gemv_lds_bytes(rows, K, ZW))
    _lib.check(_forward_rows(L.awq_gemv_forward, x2d, qweight, scales, qzeros, y, chunk, K, N, group_size, ZW, flags), "awq_gemv_forward")
    return y


def gemv_auto_kernel(M, K, N, group_size):
    """Which AWQ_GEMV_KERNEL_* awq_gemv_forward's AUTO dispatch takes for this shape (host only; -1: none)."""
    return int(_lib.lib().awq_gemv_auto_kernel(M, K, N, group_size))


GEMV_EX_SILU_PAIRS = 1  # include/awq_hip.h AWQ_GEMV_EX_SILU_PAIRS
GEMV_KERNEL_PREFILL = 4  # include/awq_hip.h AWQ_GEMV_KERNEL_PREFILL
GEMV_KERNEL_BATCH = 5    # include/awq_hip.h AWQ_GEMV_KERNEL_BATCH


def gemv_forward_ex(x2d, qweight, scales, qzeros, group_size, norm_weight=None, norm_eps=0.0, add_residual=None,
                    silu_pairs=False):
    """GEMV-layout decode projection with the decoder block's prologue / epilogue in the same launch
    (awq_gemv_forward_ex): norm_weight normalises x on its way into registers; add_residual stores
    fp16(fp16(W x) + add_residual); silu_pairs: rows (2 i, 2 i + 1) are (gate_i, up_i), returns [1, N / 2] =
    silu(gate) * up.  Raises AwqHipError with code AWQ_ERR_UNSUPPORTED (-3) for shapes the row-streaming kernel
    does not take (M > 1, K > 16384): the caller then runs the separate launches."""
    _require_gpu(norm_weight, add_residual)
    x2d, qweight, scales, qzeros, y, M, K, N, ZW = _gemv_operands("gemv_forward_ex", x2d, qweight, scales, qzeros, halve=silu_pairs)
    if add_residual is not None and (add_residual.shape != y.shape or add_residual.dtype != torch.float16
                                     or not add_residual.is_contiguous()):
        raise _lib.AwqHipError("gemv_forward_ex: add_residual must be a contiguous fp16 [M, N] tensor")
    if norm_weight is not None and (norm_weight.dtype != torch.float16 or norm_weight.numel() != K):
        raise _lib.AwqHipError("gemv_forward_ex: norm_weight must be fp16 [K]")
    with torch.cuda.device(x2d.device):
        e = _lib.AwqGemvEx()
        e.struct_bytes = ctypes.sizeof(_lib.AwqGemvEx)
        e.flags = GEMV_EX_SILU_PAIRS if silu_pairs else 0
        e.x, e.qweight, e.scales, e.qzeros, e.y = _ptr(x2d), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(y)
        e.M, e.K, e.N, e.group_size, e.zeros_width = M, K, N, group_size, ZW
        e.stream = _stream()
        e.norm_weight = _ptr(norm_weight.contiguous()) if norm_weight is not None else None
        e.norm_eps = float(norm_eps)
        e.add_residual = _ptr(add_residual)
        rc = _lib.lib().awq_gemv_forward_ex(ctypes.byref(e))
    _lib.check(rc, "awq_gemv_forward_ex")
    return y


def _dequantize_nk(name, qweight, scales, qzeros, N, K, *sizes):
    """fp16 W^T [N, K] of GEMV- or GEMVFast-layout buffers by the library's dequantiser `name`"""
    _require_gpu(qweight, scales, qzeros)
    qweight, scales, qzeros = qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    out = torch.empty((N, K), dtype=torch.float16, device=qweight.device)
    with torch.cuda.device(qweight.device):
        _lib.check(getattr(_lib.lib(), name)(_ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(out), K, N, *sizes, _stream()), name)
    return out


def dequantize_weights_gemv(qweight, scales, qzeros, group_size):
    """GEMV-layout buffers -> fp16 W^T [N, K] (awq_dequantize_weights_gemv)."""
    return _dequantize_nk("awq_dequantize_weights_gemv", qweight, scales, qzeros, qweight.shape[0], qweight.shape[1] * 8, group_size,
                          qzeros.shape[1])


def repack_gemv_to_gemm(qweight, scales, qzeros, group_size):
    """GEMV-layout buffers -> (qweight [K, N/8], scales [K/g, N], qzeros [K/g, N/8]) in the GEMM layout: the same integers and
    scales, bit for bit (awq_repack_gemv_to_gemm, csrc/repack.hip).  The outputs are fresh temporaries."""
    _require_gpu(qweight, scales, qzeros)
    qweight, scales, qzeros = qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    N, K = qweight.shape[0], qweight.shape[1] * 8
    G = K // group_size
    qw = torch.empty((K, N // 8), dtype=torch.int32, device=qweight.device)
    sc = torch.empty((G, N), dtype=torch.float16, device=qweight.device)
    qz = torch.empty((G, N // 8), dtype=torch.int32, device=qweight.device)
    with torch.cuda.device(qweight.device):
        _lib.check(_lib.lib().awq_repack_gemv_to_gemm(_ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(qw), _ptr(sc), _ptr(qz), K, N,
                                                      group_size, qzeros.shape[1], _stream()), "awq_repack_gemv_to_gemm")
    return qw, sc, qz


REPACK_DEINTERLEAVE_HALVES = 1  # include/awq_hip.h AWQ_REPACK_DEINTERLEAVE_HALVES

_expert_workspaces = {}  # device index -> uint8 buffer: the GEMM-layout temporary of single-copy expert stacks


def expert_workspace(device, E, K, N, G):
    """(qweight [E, K, N/8] i32, scales [E, G, N] f16, qzeros [E, G, N/8] i32): views of ONE persistent buffer per device, grown to
    the largest expert stack seen there and shared by every layer and both projections of every single-copy MoE block
    (modules/fused/moe.py) -- work on one stream runs in order, so the next repack only overwrites weights the GEMM before it has
    read.  Never (re)allocated while a hipGraph is being captured: a captured step has to find it in place (GraphedDecoder's
    warm-up step allocates it).  An outgrown buffer is retired, not freed: a graph captured earlier may still replay into it."""
    nq, ns, nz = E * K * (N // 8) * 4, E * G * N * 2, E * G * (N // 8) * 4
    oq, os_ = (nq + 255) & ~255, (ns + 255) & ~255
    need = oq + os_ + nz
    key = device.index if device.index is not None else torch.cuda.current_device()
    buf = _expert_workspaces.get(key)
    if buf is None or buf.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.AwqHipError(f"expert_workspace: {need} bytes needed on device {key} while a hipGraph is being captured; run "
                                   "the step once outside the capture first (GraphedDecoder's warm-up does)")
        if buf is not None:
            _retired_raw.append(buf)
        with torch.inference_mode(False):
            buf = torch.empty(need, dtype=torch.uint8, device=device)
        _expert_workspaces[key] = buf
    return (buf[:nq].view(torch.int32).view(E, K, N // 8), buf[oq:oq + ns].view(torch.float16).view(E, G, N),
            buf[oq + os_:oq + os_ + nz].view(torch.int32).view(E, G, N // 8))


def repack_gemv_stack_to_gemm(qweight, scales, qzeros, group_size, out=None, seg_offsets=None, topk_ids=None,
                              deinterleave_halves=False):
    """A GEMV-layout expert stack (qweight [E, N, K/8], qzeros [E, N, ZW], scales [E, N, 8 ZW]: utils/convert.py::gemm_stack_to_gemv)
    -> (qweight [E, K, N/8], scales [E, K/g, N], qzeros [E, K/g, N/8]) in the GEMM layout, bit for bit
    (awq_repack_gemv_stack_to_gemm, csrc/repack.hip).  out: the three caller-owned buffers (default: the device's
    expert_workspace).  Only the experts with rows in seg_offsets [E + 1] (moe_sort_pairs) / occurring in topk_ids are converted,
    picked on the device; the others' parts of `out` are not written.  deinterleave_halves: the inverse of
    gemm_stack_to_gemv(interleave_halves=True)."""
    _require_gpu(qweight, scales, qzeros, seg_offsets, topk_ids)
    qweight, scales, qzeros = qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    E, N, KW = qweight.shape
    K, ZW = KW * 8, qzeros.shape[2]
    if group_size <= 0 or K % group_size or qzeros.shape[:2] != (E, N) or scales.shape != (E, N, ZW * 8):
        raise _lib.AwqHipError(f"repack_gemv_stack_to_gemm: shape mismatch qweight{tuple(qweight.shape)} qzeros{tuple(qzeros.shape)} "
                               f"scales{tuple(scales.shape)} group_size {group_size}")
    G = K // group_size
    qw, sc, qz = out if out is not None else expert_workspace(qweight.device, E, K, N, G)
    if (qw.shape != (E, K, N // 8) or sc.shape != (E, G, N) or qz.shape != (E, G, N // 8) or qw.dtype != torch.int32
            or sc.dtype != torch.float16 or qz.dtype != torch.int32 or not (qw.is_contiguous() and sc.is_contiguous() and qz.is_contiguous())
            or qw.device != qweight.device or sc.device != qweight.device or qz.device != qweight.device):
        raise _lib.AwqHipError("repack_gemv_stack_to_gemm: out must be contiguous (int32 [E, K, N/8], fp16 [E, K/g, N], int32 [E, K/g, N/8]) "
                               "on the stack's device")
    pairs = 0
    for name, t, n in (("seg_offsets", seg_offsets, E + 1), ("topk_ids", topk_ids, None)):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or (n is not None and t.numel() != n)):
            raise _lib.AwqHipError(f"repack_gemv_stack_to_gemm: {name} must be a contiguous int32 tensor" + (f" of {n}" if n else ""))
    if topk_ids is not None:
        pairs = topk_ids.numel()
        if pairs == 0:  # no pair, no expert (an empty tensor has no pointer to tell the library so)
            return qw, sc, qz
    with torch.cuda.device(qweight.device):
        rc = _lib.lib().awq_repack_gemv_stack_to_gemm(_ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(qw), _ptr(sc), _ptr(qz),
                                                      _ptr(seg_offsets), _ptr(topk_ids), pairs, E, K, N, group_size, ZW,
                                                      REPACK_DEINTERLEAVE_HALVES if deinterleave_halves else 0, _stream())
    _lib.check(rc, "awq_repack_gemv_stack_to_gemm")
    return qw, sc, qz


def gemv_prefill_repack(x2d, qweight, scales, qzeros, group_size, bias=None):
    """Prefill-sized batches on the GEMV layout's own buffers: transpose the packed nibbles into a temporary of this call
    (repack_gemv_to_gemm) and run the fused MFMA GEMM on it (gemm_forward) -- two hand-written launches, nothing resident."""
    qw, sc, qz = repack_gemv_to_gemm(qweight, scales, qzeros, group_size)
    return gemm_forward(x2d, qw, sc, qz, bias)


def silu_and_mul(gate_up, out=None):
    """[..., 2d] fp16 = [gate | up] -> [..., d] = silu(gate) * up (awq_silu_and_mul)."""
    _require_gpu(gate_up)
    gate_up = gate_up.contiguous()
    d = gate_up.shape[-1] // 2
    if out is None:
        out = torch.empty(gate_up.shape[:-1] + (d,), dtype=torch.float16, device=gate_up.device)
    rows = gate_up.numel() // (2 * d) if d else 0
    with torch.cuda.device(gate_up.device):
        _lib.check(_lib.lib().awq_silu_and_mul(_ptr(gate_up), _ptr(out), rows, d, _stream()), "awq_silu_and_mul")
    return out


_moe_workspaces = {}


def grouped_gemm_forward(x, qweight, scales, qzeros, topk_weights, sorted_token_ids, expert_ids,
                         num_tokens_post_padded, mul_weights, split_k_iters=8, block_rows=16, zero_init=False, x_gated=False):
    """awq_ext.grouped_gemm_forward semantics (awq/modules/fused/moe.py:60-89): x [T, 1 | topk, K] fp16,
    stacked GEMM-layout expert tensors [E, ...]; returns [T, topk, N] fp16.  Nothing is read back
    to the host: the routing tensors are consumed on the device.  block_rows = the block size the
    routing tensors were aligned with (16 like the reference, or 8: decode-sized batches)."""
    _require_gpu(x, qweight, scales, qzeros, topk_weights, sorted_token_ids, expert_ids, num_tokens_post_padded)
    T, topk = topk_weights.shape
    E, K, NW = qweight.shape
    N = NW * 8
    G = qzeros.shape[1]
    x = x.contiguous()
    x_div = topk if x.shape[1] == 1 else 1
    # x_gated: x holds [gate | up] rows of 2 K halves; silu(gate) * up is applied while the kernel stages its activations
    if x.shape[0] * x.shape[1] * x_div != T * topk or x.shape[-1] != (2 * K if x_gated else K):
        raise _lib.AwqHipError(f"grouped_gemm_forward: x{tuple(x.shape)} does not match {T} tokens x top-{topk}")
    qweight, scales, qzeros = qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    sorted_token_ids = sorted_token_ids.contiguous()
    # zero_init: rows of pairs that no block covers (expert-parallel routing places only the local experts' pairs) read as 0
    y = (torch.zeros if zero_init else torch.empty)((T, topk, N), dtype=torch.float16, device=x.device)
    # expert_ids has the reference's capacity (one entry per pair + E, moe.py:121-123); the blocks that can exist are bounded by
    # the padded row capacity of sorted_token_ids: that bound sizes the grid and the split-K exchange
    max_blocks = max(1, min(expert_ids.numel(), sorted_token_ids.numel() // block_rows))
    L = _lib.lib()
    with torch.cuda.device(x.device):
        need = L.awq_grouped_gemm_workspace_bytes(max_blocks, K, N)
        key = (x.device.index, _stream())
        ws = _moe_workspaces.get(key)
        if ws is None or ws.numel() < need:
            if ws is not None:
                _retired_raw.append(ws)  # a captured graph may still replay into it
            ws = torch.empty(int(need), dtype=torch.uint8, device=x.device)
            _lib.check(L.awq_gemm_workspace_init(_ptr(ws), ws.numel(), _stream()), "awq_gemm_workspace_init")
            _moe_workspaces[key] = ws
        w = topk_weights.contiguous().float() if mul_weights else None
        rc = L.awq_grouped_gemm_forward_ex(_ptr(x), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(y),
                                           _ptr(sorted_token_ids), _ptr(expert_ids), _ptr(num_tokens_post_padded),
                                           _ptr(w), T * topk, x_div, block_rows, max_blocks, E, K, N, K // G, _ptr(ws),
                                           ws.numel(), X_GATED_SILU if x_gated else 0, _stream())
    _lib.check(rc, "awq_grouped_gemm_forward")
    return y


def grouped_gemv_forward(x, qweight, scales, qzeros, topk_ids, group_size, topk_weights=None, silu_pairs=False, parts=0,
                         zero_init=False, first_expert=0):
    """MoE decode on GEMV-layout expert stacks (awq_grouped_gemv_forward; the decode-sized calls of
    awq/modules/fused/moe.py:60-89): x [T, K] (every token feeds its topk pairs) or [T * topk, K] (one row per pair) fp16,
    qweight [E, N, K/8] i32, qzeros [E, N, ZW] i32, scales [E, N, 8 ZW] fp16, topk_ids [T, topk] i32 on the device.
    Returns [T, topk, N] (N / 2 with silu_pairs: rows (2 j, 2 j + 1) of every expert = (gate_j, up_j), silu(gate) * up
    written by the launch); topk_weights [T, topk] fp32 multiplies each pair's row before its one rounding.  One launch of
    the row-streaming kernel for all pairs; the stack holds experts [first_expert, first_expert + E) of topk_ids' global ids
    and pairs of other experts are skipped (expert-parallel shards; zero_init: their rows read as 0)."""
    _require_gpu(x, qweight, scales, qzeros, topk_ids, topk_weights)
    if x.dtype != torch.float16 or topk_ids.dtype != torch.int32:
        raise _lib.AwqHipError("grouped_gemv_forward expects fp16 activations and int32 topk_ids")
    T, topk = topk_ids.shape
    E, N, KW = qweight.shape
    K, ZW = KW * 8, qzeros.shape[2]
    P = T * topk
    x = x.contiguous()
    if x.dim() != 2 or x.shape[1] != K or x.shape[0] not in (T, P):
        raise _lib.AwqHipError(f"grouped_gemv_forward: x{tuple(x.shape)} does not match {T} tokens x top-{topk}, K = {K}")
    x_div = topk if x.shape[0] == T and topk > 1 else 1
    if qzeros.shape[:2] != (E, N) or scales.shape != (E, N, ZW * 8):
        raise _lib.AwqHipError(f"grouped_gemv_forward: shape mismatch qweight{tuple(qweight.shape)} qzeros{tuple(qzeros.shape)} "
                               f"scales{tuple(scales.shape)}")
    qweight, scales, qzeros, topk_ids = qweight.contiguous(), scales.contiguous(), qzeros.contiguous(), topk_ids.contiguous()
    w = topk_weights.contiguous().float() if topk_weights is not None else None
    if w is not None and w.numel() != P:
        raise _lib.AwqHipError("grouped_gemv_forward: topk_weights must hold one weight per pair")
    y = (torch.zeros if zero_init else torch.empty)((T, topk, N // 2 if silu_pairs else N), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().awq_grouped_gemv_forward(_ptr(x), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(y), _ptr(topk_ids),
                                                 _ptr(w), P, x_div, E, first_expert, K, N, group_size, ZW,
                                                 GEMV_EX_SILU_PAIRS if silu_pairs else 0, parts, _stream())
    _lib.check(rc, "awq_grouped_gemv_forward")
    return y


def moe_route(gating_output, topk, renormalize, block_size, first_expert=0, num_local=None):
    """softmax + top-k (+ renormalise) + block alignment in ONE launch (awq_moe_route): returns
    (topk_weights [T, k] fp32, topk_ids [T, k] i32, sorted_token_ids, expert_ids, num_tokens_post_padded).
    block_size = 0: routing only (the last three are None).
    first_expert / num_local (expert parallel, awq_moe_route_local): only the pairs of experts
    [first_expert, first_expert + num_local) are placed, expert_ids are relative to first_expert; topk_ids stay global."""
    _require_gpu(gating_output)
    g = gating_output.float().contiguous()
    T, E = g.shape
    nl = E if num_local is None else num_local
    dev = g.device
    w = torch.empty((T, topk), dtype=torch.float32, device=dev)
    ids = torch.empty((T, topk), dtype=torch.int32, device=dev)
    if block_size == 0:  # routing only: no alignment pass (the row-streaming MoE decode path runs pairs, not blocks)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().awq_moe_route_local(_ptr(g), _ptr(w), _ptr(ids), None, None, None, T, E, topk,
                                                      1 if renormalize else 0, 0, first_expert, nl, _stream()), "awq_moe_route_local")
        return w, ids, None, None, None
    sorted_ids = torch.empty((T * topk + nl * (block_size - 1),), dtype=torch.int32, device=dev)
    expert_ids = torch.empty((T * topk + nl,), dtype=torch.int32, device=dev)
    npad = torch.empty((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().awq_moe_route_local(_ptr(g), _ptr(w), _ptr(ids), _ptr(sorted_ids), _ptr(expert_ids), _ptr(npad), T, E,
                                                  topk, 1 if renormalize else 0, block_size, first_expert, nl, _stream()),
                   "awq_moe_route_local")
    return w, ids, sorted_ids, expert_ids, npad


def moe_align_block_size(topk_ids, block_size, num_experts):
    """Device-side (no host read) restatement of moe_align_block_size (awq/modules/fused/moe.py:94-134):
    returns (sorted_token_ids [numel + E*(block-1)] padded with `numel`, expert_ids [numel + E] one per
    block (entries past the used blocks are 0), num_tokens_post_padded [1]) as int32 tensors."""
    flat = topk_ids.reshape(-1).to(torch.int64)
    numel = flat.numel()
    dev = flat.device
    # one-hot sum instead of torch.bincount: bincount reads its output size back to the host
    counts = (flat.unsqueeze(1) == torch.arange(num_experts, device=dev).unsqueeze(0)).sum(0)
    padded = (counts + block_size - 1) // block_size * block_size
    pad_end = torch.cumsum(padded, 0)
    pad_start = pad_end - padded
    raw_start = torch.cumsum(counts, 0) - counts
    order = torch.argsort(flat, stable=True)                 # pairs grouped by expert, original order kept
    e_sorted = flat[order]
    rank = torch.arange(numel, device=dev) - raw_start[e_sorted]
    pos = pad_start[e_sorted] + rank
    sorted_ids = torch.full((numel + num_experts * (block_size - 1),), numel, dtype=torch.int32, device=dev)
    sorted_ids[pos] = order.to(torch.int32)
    nblk = numel + num_experts  # capacity used by the reference (moe.py:121-123)
    blk_first_row = torch.arange(nblk, device=dev) * block_size
    expert_ids = torch.searchsorted(pad_end, blk_first_row, right=True).clamp_(max=num_experts - 1).to(torch.int32)
    return sorted_ids, expert_ids, pad_end[-1:].to(torch.int32)


def fused_topk(gating_output, topk, renormalize):
    """awq/modules/fused/moe.py:137-171 (the branch the reference itself takes on ROCm)."""
    routing = torch.softmax(gating_output, dim=-1, dtype=torch.float32)
    w, ids = torch.topk(routing, topk, dim=-1)
    if renormalize:
        w = w / w.sum(dim=-1, keepdim=True)
    return w, ids.to(torch.int32)


def _gemv_fast_operands(name, x2d, qweight, scales, qzeros):
    """GEMVFast layout: as _gemv_operands; (x2d, qweight, scales, qzeros, y, M, K, N, GP), GP = the rows of scales / qzeros"""
    _require_gpu(x2d, qweight, scales, qzeros)
    if x2d.dtype != torch.float16:
        raise _lib.AwqHipError(f"{name} expects fp16 activations")
    x2d, qweight, scales, qzeros = x2d.contiguous(), qweight.contiguous(), scales.contiguous(), qzeros.contiguous()
    M, K = x2d.shape
    N, GP = qweight.shape[0] * 4, scales.shape[0]
    if qweight.shape[1] != K or scales.shape != (GP, N) or qzeros.shape != (GP, N):
        raise _lib.AwqHipError(f"{name}: shape mismatch x{tuple(x2d.shape)} qweight{tuple(qweight.shape)} "
                               f"scales{tuple(scales.shape)}")
    y = torch.empty((M, N), dtype=torch.float16, device=x2d.device)
    return x2d, qweight, scales, qzeros, y, M, K, N, GP


def gemv_fast_forward(x2d, qweight, scales, qzeros, group_size, flags=0):
    """GEMVFast layout (qweight int16 [N/4, K], scales / qzeros fp16 [8*ZW, N]): y [M, N] fp16
    (awq_gemv_fast_forward).  AUTO: the batched kernel (csrc/gemv_batch.hip, GEMVFast form) from five rows -- at every batch size while
    2048 < K <= 4096 -- in one call; otherwise the 16-row kernel (csrc/gemv_fast.hip) in chunks of <= 16 rows."""
    x2d, qweight, scales, qzeros, y, M, K, N, GP = _gemv_fast_operands("gemv_fast_forward", x2d, qweight, scales, qzeros)
    if M == 0:
        return y
    L = _lib.lib()

    def run(chunk):
        return _forward_rows(L.awq_gemv_fast_forward, x2d, qweight, scales, qzeros, y, chunk, K, N, group_size, GP, flags)

    kern = flags & 0xF
    if kern == GEMV_KERNEL_BATCH or (kern == 0 and M >= 5):
        # the batched kernel in its GEMVFast form takes ANY M in one call (launches of <= 128 rows inside the library); shapes it
        # refuses (group sizes other than 128) fall through to the 16-row kernel in chunks, unless the caller named it
        rc = run(M)
        if rc != _lib.ERR_UNSUPPORTED or kern == GEMV_KERNEL_BATCH:
            _lib.check(rc, "awq_gemv_fast_forward")
            return y
    _lib.check(run(_decode_chunk(lambda rows: L.awq_gemv_fast_lds_bytes_c(rows, K, group_size))), "awq_gemv_fast_forward")
    return y


def gemv_fast_prefill(x2d, qweight, scales, qzeros, group_size, flags=0):
    """GEMVFast layout, prefill-sized token counts: y [M, N] = x @ W^T, W = fp16(w * s + qzeros), by TWO hand-written launches
    (awq_gemv_fast_prefill: the packed words transposed into a temporary of the call, then the register-decoded MFMA GEMM with this
    format's scales / fp16 zero terms) -- the role of awq_v2_ext.gemm_forward_cuda_prefill (awq/modules/linear/gemv_fast.py:203-206).
    Raises AwqHipError with code ERR_UNSUPPORTED for shapes the fused kernel does not take (K % 64, group_size % 64, N % 8)."""
    x2d, qweight, scales, qzeros, y, M, K, N, GP = _gemv_fast_operands("gemv_fast_prefill", x2d, qweight, scales, qzeros)
    if M == 0:
        return y
    tmp = torch.empty((K, max(N // 8, 1)), dtype=torch.int32, device=x2d.device)  # GEMM-layout words of the same integers: a temporary of the call
    with torch.cuda.device(x2d.device):
        rc = _lib.lib().awq_gemv_fast_prefill(_ptr(x2d), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(y), _ptr(tmp), M, K, N, group_size, GP,
                                              flags, _stream())
    _lib.check(rc, "awq_gemv_fast_prefill")
    return y


def repack_gemvfast_to_gemm(qweight):
    """GEMVFast words int16 [N/4, K] -> GEMM-layout words int32 [K, N/8] (awq_repack_gemvfast_to_gemm), bit-exact"""
    _require_gpu(qweight)
    qweight = qweight.contiguous()
    N, K = qweight.shape[0] * 4, qweight.shape[1]
    out = torch.empty((K, N // 8), dtype=torch.int32, device=qweight.device)
    with torch.cuda.device(qweight.device):
        _lib.check(_lib.lib().awq_repack_gemvfast_to_gemm(_ptr(qweight), _ptr(out), K, N, _stream()), "awq_repack_gemvfast_to_gemm")
    return out


def dequantize_weights_gemv_fast(qweight, scales, qzeros, group_size):
    """GEMVFast-layout buffers -> fp16 W^T [N, K] (awq_dequantize_weights_gemv_fast)."""
    return _dequantize_nk("awq_dequantize_weights_gemv_fast", qweight, scales, qzeros, qweight.shape[0] * 4, qweight.shape[1], group_size)


def auto_kernel(M, K, N, group_size):
    """KERNEL_* the AUTO dispatch of gemm_forward takes for this shape (host-only query, no launch)."""
    return _lib.lib().awq_gemm_auto_kernel(M, K, N, group_size)


def last_kernel():
    return _lib.lib().awq_hip_last_kernel().decode()


# ---- fused decoder block (csrc/decoder.hip)
def rmsnorm(x, weight, eps, residual=None, out=None):
    """out = rmsnorm(x) * weight (awq_rmsnorm_forward); with `residual` (same shape, updated in place):
    residual += x, out = rmsnorm(residual) * weight."""
    _require_gpu(x, weight, residual)
    if x.dtype != torch.float16 or weight.dtype != torch.float16:
        raise _lib.AwqHipError("rmsnorm expects fp16 tensors")
    x = x.contiguous()
    H = x.shape[-1]
    M = x.numel() // H if H else 0
    if out is None:
        out = torch.empty_like(x)
    if residual is not None and (not residual.is_contiguous() or residual.shape != x.shape or residual.dtype != x.dtype):
        raise _lib.AwqHipError("rmsnorm: residual must be a contiguous fp16 tensor of x's shape")
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awq_rmsnorm_forward(_ptr(x), _ptr(residual), _ptr(weight.contiguous()), _ptr(out), M, H,
                                                  float(eps), _stream()), "awq_rmsnorm_forward")
    return out


def _check_rows(name, what, rows, shared, B, device):
    """The per-row position / length words of the *_rows entry points: int32 [B] on the kernel's device, not combined with the
    shared word."""
    if shared is not None:
        raise _lib.AwqHipError(f"{name}: {what}_rows and the shared device word cannot be combined")
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or not rows.is_cuda or rows.device != device:
        raise _lib.AwqHipError(f"{name}: {what}_rows must be an int32 tensor on {device}")
    if tuple(rows.shape) != (B,) or not rows.is_contiguous():
        raise _lib.AwqHipError(f"{name}: {what}_rows must be a contiguous [{B}] tensor, got {tuple(rows.shape)}")


def _kv8(name, k_cache, v_cache, k_scale, v_scale):
    """True for an fp8 cache (uint8 codes [B, Tmax, Hkv, 128] + fp32 scales [B, Tmax, Hkv], include/awq_hip.h), False for
    fp16; a uint8 cache without its scales, or scales next to an fp16 cache, is an error."""
    codes = k_cache.dtype == torch.uint8 or v_cache.dtype == torch.uint8
    scales = k_scale is not None or v_scale is not None
    if not codes and not scales:
        return False
    if not codes:
        raise _lib.AwqHipError(f"{name}: k_scale / v_scale belong to an fp8 (uint8) cache, got {k_cache.dtype}")
    if k_scale is None or v_scale is None:
        raise _lib.AwqHipError(f"{name}: an fp8 (uint8) cache needs both k_scale and v_scale")
    if k_cache.dtype != v_cache.dtype:
        raise _lib.AwqHipError(f"{name}: k and v caches differ in dtype ({k_cache.dtype}, {v_cache.dtype})")
    for sc, c in ((k_scale, k_cache), (v_scale, v_cache)):
        if sc.dtype != torch.float32 or not sc.is_contiguous() or tuple(sc.shape) != tuple(c.shape[:3]):
            raise _lib.AwqHipError(f"{name}: scales must be contiguous fp32 {tuple(c.shape[:3])}, got {sc.dtype} {tuple(sc.shape)}")
        if sc.device != c.device:
            raise _lib.AwqHipError(f"{name}: scales and cache on different devices")
    return True


def _kv_ptrs(kv8, k_cache, v_cache, k_scale, v_scale):
    """the cache arguments of an attention entry point: the *_fp8 forms take the scale arrays after the caches"""
    return [_ptr(k_cache), _ptr(v_cache)] + ([_ptr(k_scale), _ptr(v_scale)] if kv8 else [])


def _stream_workspace(table, device, need):
    """The scratch tensor of `table` for (device, current stream), at least `need` bytes.  One that has to grow retires the old
    tensor into _retired_raw: a captured graph may still hold it."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    ws = table.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            _retired_raw.append(ws)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        table[key] = ws
    return ws


def rope_kv_append(qkv, k_cache, v_cache, cos, sin, start_pos, n_heads, n_kv_heads, head_dim, rotary_dim, pos_dev=None,
                   pos_rows=None, k_scale=None, v_scale=None, count_rows=None):
    """qkv [B, S, (Hq + 2 Hkv) * D] fp16 -> rotated q [B, S, Hq, D]; rotated k and v are written into
    the caches [B, Tmax, Hkv, D] at rows start_pos .. start_pos + S - 1 (awq_rope_kv_append).  pos_rows (int32 [B] on the
    device; start_pos is then ignored): sequence b starts at pos_rows[b] (awq_rope_kv_append_rows).  k_scale / v_scale
    ([B, Tmax, Hkv] fp32) with uint8 caches: the fp8 cache -- rows are stored as e4m3 codes + scales (awq_rope_kv_append*_fp8).
    count_rows (int32 [B] on the device, with pos_rows): sequence b has count_rows[b] new tokens; the slots behind them write
    nothing to the caches and their q is unspecified (awq_rope_kv_append_rows_n*)."""
    kv8 = _kv8("rope_kv_append", k_cache, v_cache, k_scale, v_scale)
    _require_gpu(qkv, k_cache, v_cache, cos, sin, pos_dev, pos_rows, k_scale, v_scale)
    B, S = qkv.shape[0], qkv.shape[1]
    qkv = qkv.contiguous()
    q = torch.empty((B, S, n_heads, head_dim), dtype=torch.float16, device=qkv.device)
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()) or k_cache.shape[0] < B:
        raise _lib.AwqHipError("rope_kv_append: caches must be contiguous [>=B, Tmax, Hkv, D]")
    rows = pos_rows is not None
    if rows:
        _check_rows("rope_kv_append", "pos", pos_rows, pos_dev, B, qkv.device)
    counts = count_rows is not None
    if counts:
        if not rows:
            raise _lib.AwqHipError("rope_kv_append: count_rows goes with pos_rows")
        _check_rows("rope_kv_append", "count", count_rows, None, B, qkv.device)
    name = "awq_rope_kv_append" + ("_rows" if rows else "") + ("_n" if counts else "") + ("_fp8" if kv8 else "")
    with torch.cuda.device(qkv.device):
        _lib.check(getattr(_lib.lib(), name)(
            _ptr(qkv), _ptr(q), *_kv_ptrs(kv8, k_cache, v_cache, k_scale, v_scale), _ptr(cos), _ptr(sin),
            *([_ptr(pos_rows)] + ([_ptr(count_rows)] if counts else []) if rows else [_ptr(pos_dev), int(start_pos)]),
            B, S, n_heads, n_kv_heads, head_dim, rotary_dim, k_cache.shape[1], _stream()), name)
    return q


def prefill_attention(q, k_cache, v_cache, start_pos, scale=None, softcap=0.0, alibi_slopes=None):
    """q [B, S, Hq, 128] fp16 (after RoPE), caches [>= B, Tmax, Hkv, 128] fp16 already holding rows 0 .. start_pos + S - 1 ->
    [B, S, Hq, 128]: causal attention of the S new rows over the cache (awq_prefill_attention, csrc/prefill_attn.hip; the
    reference's flash_attn_func call, attn.py:269-277).  Raises AwqHipError code -3 for head sizes other than 128."""
    _require_gpu(q, k_cache, v_cache, alibi_slopes)
    if q.dtype != torch.float16 or k_cache.dtype != torch.float16 or v_cache.dtype != torch.float16:
        raise _lib.AwqHipError("prefill_attention expects fp16 tensors")
    B, S, Hq, D = q.shape
    Tmax, Hkv = k_cache.shape[1], k_cache.shape[2]
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()) or k_cache.shape[0] < B or k_cache.shape != v_cache.shape:
        raise _lib.AwqHipError("prefill_attention: caches must be contiguous [>=B, Tmax, Hkv, D]")
    q = q.contiguous()
    out = torch.empty_like(q)
    if alibi_slopes is not None:
        alibi_slopes = alibi_slopes.to(torch.float32).contiguous()
        if alibi_slopes.numel() != Hq:
            raise _lib.AwqHipError("prefill_attention: alibi_slopes must have one entry per query head")
    if scale is None:
        scale = D ** -0.5
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().awq_prefill_attention(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, S, Hq, Hkv, D, Tmax, int(start_pos),
                                                    float(scale), float(softcap), _ptr(alibi_slopes), _stream()), "awq_prefill_attention")
    return out


def prefill_attention_rows(q, k_cache, v_cache, pos_rows, count_rows, max_end, scale=None, softcap=0.0, alibi_slopes=None, out=None):
    """prefill_attention with one start and one count per sequence (int32 [B] on the device): query (b, s), s < count_rows[b],
    sees cache rows <= pos_rows[b] + s; the slots behind them are not written -- `out` (default: zeros) keeps what it held
    there.  max_end: the host's bound of pos_rows[b] + count_rows[b], <= Tmax (awq_prefill_attention_rows)."""
    _require_gpu(q, k_cache, v_cache, alibi_slopes, pos_rows, count_rows, out)
    if q.dtype != torch.float16 or k_cache.dtype != torch.float16 or v_cache.dtype != torch.float16:
        raise _lib.AwqHipError("prefill_attention_rows expects fp16 tensors")
    B, S, Hq, D = q.shape
    Tmax, Hkv = k_cache.shape[1], k_cache.shape[2]
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()) or k_cache.shape[0] < B or k_cache.shape != v_cache.shape:
        raise _lib.AwqHipError("prefill_attention_rows: caches must be contiguous [>=B, Tmax, Hkv, D]")
    _check_rows("prefill_attention_rows", "pos", pos_rows, None, B, q.device)
    _check_rows("prefill_attention_rows", "count", count_rows, None, B, q.device)
    q = q.contiguous()
    if out is None:
        out = torch.zeros_like(q)
    elif out.shape != q.shape or out.dtype != q.dtype or not out.is_contiguous():
        raise _lib.AwqHipError("prefill_attention_rows: out must be a contiguous fp16 tensor of q's shape")
    if alibi_slopes is not None:
        alibi_slopes = alibi_slopes.to(torch.float32).contiguous()
        if alibi_slopes.numel() != Hq:
            raise _lib.AwqHipError("prefill_attention_rows: alibi_slopes must have one entry per query head")
    if scale is None:
        scale = D ** -0.5
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().awq_prefill_attention_rows(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), _ptr(pos_rows),
                                                         _ptr(count_rows), int(max_end), B, S, Hq, Hkv, D, Tmax, float(scale),
                                                         float(softcap), _ptr(alibi_slopes), _stream()), "awq_prefill_attention_rows")
    return out


_attn_workspaces = {}


def decode_attention(q, k_cache, v_cache, seq_len, scale=None, len_dev=None, max_len=None, softcap=0.0, alibi_slopes=None,
                     len_rows=None, k_scale=None, v_scale=None):
    """q [B, Hq, 128] fp16, caches [B, Tmax, Hkv, 128] -> [B, Hq, 128]: attention of ONE query token per
    sequence over cache rows [0, seq_len) (awq_decode_attention; with logit soft-capping / ALiBi slopes [Hq] fp32:
    awq_decode_attention_ex).  len_rows (int32 [B] on the device; seq_len is then ignored): sequence b attends over rows
    [0, len_rows[b]), the launch sized for max_len (default: the cache window) -- awq_decode_attention_rows.  k_scale /
    v_scale with uint8 caches: the fp8 cache (the *_fp8 entry points)."""
    kv8 = _kv8("decode_attention", k_cache, v_cache, k_scale, v_scale)
    _require_gpu(q, k_cache, v_cache, len_dev, alibi_slopes, len_rows, k_scale, v_scale)
    B, Hq, D = q.shape
    Hkv, Tmax = k_cache.shape[2], k_cache.shape[1]
    q = q.contiguous()
    out = torch.empty_like(q)
    ws = _stream_workspace(_attn_workspaces, q.device, _lib.lib().awq_decode_attention_workspace_bytes(B, Hq))
    if scale is None:
        scale = D ** -0.5
    if alibi_slopes is not None:
        alibi_slopes = alibi_slopes.to(torch.float32).contiguous()
        if alibi_slopes.numel() != Hq:
            raise _lib.AwqHipError("decode_attention: alibi_slopes must hold one slope per query head")
    rows = len_rows is not None
    if rows:
        _check_rows("decode_attention", "len", len_rows, len_dev, B, q.device)
    # the rows and fp8 forms take softcap / alibi_slopes themselves; fp16 with the shared word has the _ex entry for them
    extra = rows or kv8 or bool(softcap) or alibi_slopes is not None
    name = "awq_decode_attention" + ("_rows" if rows else "_ex" if extra else "") + ("_fp8" if kv8 else "")
    if max_len is None:
        max_len = Tmax if rows else seq_len
    with torch.cuda.device(q.device):
        _lib.check(getattr(_lib.lib(), name)(
            _ptr(q), *_kv_ptrs(kv8, k_cache, v_cache, k_scale, v_scale), _ptr(out),
            *([_ptr(len_rows)] if rows else [_ptr(len_dev), int(seq_len)]), int(max_len),
            B, Hq, Hkv, D, Tmax, float(scale), *([float(softcap), _ptr(alibi_slopes)] if extra else []),
            _ptr(ws), ws.numel(), _stream()), name)
    return out


def decode_attention_rope(qkv, k_cache, v_cache, cos, sin, start_pos, n_heads, n_kv_heads, pos_dev=None, max_len=None,
                          scale=None, pos_rows=None, k_scale=None, v_scale=None):
    """One launch for a decode step: qkv [B, 1, (Hq + 2 Hkv) * 128] (or [B, ...]) -> attention output
    [B, Hq, 128]; rotates q / k, appends k / v at row start_pos and attends over rows [0, start_pos]
    (awq_decode_attention_rope; bit-identical to rope_kv_append + decode_attention).  pos_rows (int32 [B] on the device;
    start_pos is then ignored): sequence b at position pos_rows[b], the launch sized for max_len (default: the cache window)
    -- awq_decode_attention_rope_rows.  k_scale / v_scale with uint8 caches: the fp8 cache -- the new token is quantized,
    appended as codes + scales and attended to in its quantized form (the *_fp8 entry points)."""
    kv8 = _kv8("decode_attention_rope", k_cache, v_cache, k_scale, v_scale)
    _require_gpu(qkv, k_cache, v_cache, cos, sin, pos_dev, pos_rows, k_scale, v_scale)
    B = qkv.shape[0]
    D = k_cache.shape[3]
    qkv = qkv.contiguous()
    out = torch.empty((B, n_heads, D), dtype=torch.float16, device=qkv.device)
    ws = _stream_workspace(_attn_workspaces, qkv.device, _lib.lib().awq_decode_attention_workspace_bytes(B, n_heads))
    if scale is None:
        scale = D ** -0.5
    rows = pos_rows is not None
    if rows:
        _check_rows("decode_attention_rope", "pos", pos_rows, pos_dev, B, qkv.device)
    name = "awq_decode_attention_rope" + ("_rows" if rows else "") + ("_fp8" if kv8 else "")
    if max_len is None:
        max_len = k_cache.shape[1] if rows else start_pos + 1
    with torch.cuda.device(qkv.device):
        _lib.check(getattr(_lib.lib(), name)(
            _ptr(qkv), *_kv_ptrs(kv8, k_cache, v_cache, k_scale, v_scale), _ptr(cos), _ptr(sin), _ptr(out),
            *([_ptr(pos_rows)] if rows else [_ptr(pos_dev), int(start_pos)]), int(max_len),
            B, n_heads, n_kv_heads, D, k_cache.shape[1], float(scale), _ptr(ws), ws.numel(), _stream()), name)
    return out


def kv_quant_fp8(x, cache, scales, start_pos=0):
    """x [B, S, Hkv, 128] fp16 -> e4m3 codes and scales of rows [start_pos, start_pos + S) of the fp8 cache `cache` [>= B, Tmax,
    Hkv, 128] uint8 / `scales` [>= B, Tmax, Hkv] fp32, in place (awq_kv_quant_fp8; format: include/awq_hip.h)."""
    _require_gpu(x, cache, scales)
    if x.dtype != torch.float16 or cache.dtype != torch.uint8 or scales.dtype != torch.float32:
        raise _lib.AwqHipError("kv_quant_fp8 expects fp16 rows, a uint8 cache and fp32 scales")
    if x.dim() != 4 or cache.dim() != 4 or tuple(scales.shape) != tuple(cache.shape[:3]) or x.shape[0] > cache.shape[0] \
            or tuple(x.shape[2:]) != tuple(cache.shape[2:]) or not (cache.is_contiguous() and scales.is_contiguous()):
        raise _lib.AwqHipError(f"kv_quant_fp8: shapes {tuple(x.shape)}, {tuple(cache.shape)}, {tuple(scales.shape)} do not fit")
    x = x.contiguous()
    B, S, Hkv, D = x.shape
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().awq_kv_quant_fp8(_ptr(x), _ptr(cache), _ptr(scales), B, S, Hkv, D, cache.shape[1], int(start_pos),
                                               _stream()), "awq_kv_quant_fp8")


def kv_dequant_fp8(cache, scales, n, batch=None):
    """Rows [0, n) of the first `batch` sequences (default: all) of an fp8 cache -> fp16 [batch, n, Hkv, 128] =
    fp16(code * scale), saturated to +-65504 (awq_kv_dequant_fp8)."""
    _require_gpu(cache, scales)
    if cache.dtype != torch.uint8 or scales.dtype != torch.float32 or cache.dim() != 4 \
            or tuple(scales.shape) != tuple(cache.shape[:3]) or not (cache.is_contiguous() and scales.is_contiguous()):
        raise _lib.AwqHipError("kv_dequant_fp8 expects a contiguous uint8 cache [B, Tmax, Hkv, 128] and fp32 scales [B, Tmax, Hkv]")
    B = cache.shape[0] if batch is None else int(batch)
    if B > cache.shape[0]:
        raise _lib.AwqHipError(f"kv_dequant_fp8: batch {B} > cache batch {cache.shape[0]}")
    out = torch.empty((B, int(n), cache.shape[2], cache.shape[3]), dtype=torch.float16, device=cache.device)
    with torch.cuda.device(cache.device):
        _lib.check(_lib.lib().awq_kv_dequant_fp8(_ptr(cache), _ptr(scales), _ptr(out), B, int(n), cache.shape[2], cache.shape[3],
                                                 cache.shape[1], _stream()), "awq_kv_dequant_fp8")
    return out


def gemm_forward_normed(x2d, norm_weight, eps, qweight, scales, qzeros, bias=None, residual=None, flags=0):
    """(y, stream) with y [M, N] = rmsnorm(x2d (+ residual)) * norm_weight @ W and stream = fp16(x2d + residual)
    (None without a residual): awq_gemm_forward_normed, decode batches (M <= 4) of GEMM-layout weights."""
    _require_gpu(norm_weight, bias, residual)
    x2d, qweight, scales, qzeros, y, M, K, N, g = _gemm_operands("gemm_forward_normed", x2d, qweight, scales, qzeros)
    if norm_weight.numel() != K:
        raise _lib.AwqHipError("gemm_forward_normed: norm weight [K] expected")
    res_out = None
    if residual is not None:
        if residual.shape != x2d.shape or residual.dtype != torch.float16 or not residual.is_contiguous():
            raise _lib.AwqHipError("gemm_forward_normed: residual must be a contiguous fp16 tensor of x's shape")
        res_out = torch.empty_like(residual)
    with torch.cuda.device(x2d.device):
        rc = _lib.lib().awq_gemm_forward_normed(_ptr(x2d), _ptr(residual), _ptr(res_out), _ptr(norm_weight.contiguous()), float(eps),
                                                _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(bias), _ptr(y), M, K, N, g,
                                                *_gemm_workspace(x2d.device, M, K, N, g), flags, _stream())
    _lib.check(rc, "awq_gemm_forward_normed")
    return y, res_out


def gemm_forward_ex(x2d, qweight, scales, qzeros, bias=None, flags=0, norm_weight=None, norm_eps=0.0, ssq_in=None,
                    add_residual=None, want_ssq=False):
    """Decode-sized projection with the decoder block's prologue / epilogue (awq_gemm_forward_ex):
    norm_weight (+ ssq_in [M, tiles] from the producing call, else a statistic pass) normalises x while
    staging; add_residual stores y = fp16(fp16(x W + bias) + add_residual); want_ssq returns the per-tile
    sums of squares of y.  Returns (y, ssq | None)."""
    _require_gpu(bias, norm_weight, ssq_in, add_residual)
    x2d, qweight, scales, qzeros, y, M, K, N, g = _gemm_operands("gemm_forward_ex", x2d, qweight, scales, qzeros, flags & X_GATED_SILU)
    L = _lib.lib()
    ssq = torch.empty((M, L.awq_gemm_ex_ssq_tiles(N)), dtype=torch.float32, device=x2d.device) if want_ssq else None
    if add_residual is not None and (add_residual.shape != y.shape or add_residual.dtype != torch.float16
                                     or not add_residual.is_contiguous()):
        raise _lib.AwqHipError("gemm_forward_ex: add_residual must be a contiguous fp16 [M, N] tensor")
    if ssq_in is not None and (ssq_in.dtype != torch.float32 or ssq_in.shape[0] != M or not ssq_in.is_contiguous()):
        raise _lib.AwqHipError("gemm_forward_ex: ssq_in must be a contiguous fp32 [M, tiles] tensor")
    with torch.cuda.device(x2d.device):
        e = _lib.AwqGemmEx()
        e.struct_bytes = ctypes.sizeof(_lib.AwqGemmEx)
        e.flags = flags
        e.x, e.qweight, e.scales, e.qzeros, e.bias, e.y = _ptr(x2d), _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(bias), _ptr(y)
        e.M, e.K, e.N, e.group_size = M, K, N, g
        e.workspace, e.workspace_bytes = _gemm_workspace(x2d.device, M, K, N, g)
        e.stream = _stream()
        e.norm_weight = _ptr(norm_weight.contiguous()) if norm_weight is not None else None
        e.norm_eps = float(norm_eps)
        e.residual_in = e.residual_out = None
        e.ssq_in = _ptr(ssq_in)
        e.ssq_in_tiles = ssq_in.shape[1] if ssq_in is not None else 0
        e.add_residual = _ptr(add_residual)
        e.ssq_out = _ptr(ssq)
        rc = L.awq_gemm_forward_ex(ctypes.byref(e))
    _lib.check(rc, "awq_gemm_forward_ex")
    return y, ssq


# ---- token selection (csrc/sample.hip) --------------------------------------------------------------------------------
SAMPLE_FLAG_GREEDY = 1  # AWQ_SAMPLE_FLAG_GREEDY
SAMPLE_MAX_EOS = 8
_sample_workspaces = {}  # (device index, stream handle) -> zeroed uint8 tensor (every call leaves it zero)


def sample_params(*, do_sample, temperature=1.0, top_k=0, top_p=1.0, seed=0, eos_ids=(), pad=None):
    """Validate a sampling configuration and pack it as struct AwqSampleParams: a 64-byte CPU uint8 tensor the caller copies
    to the device (the kernel reads its parameters from device memory).  pad defaults to the first EOS id, else 0."""
    temperature, top_p, top_k = float(temperature), float(top_p), int(top_k)
    if top_k < 0:
        raise ValueError(f"top_k must be >= 0 (0 = off), got {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1] (1 = off), got {top_p}")
    if temperature != temperature:
        raise ValueError("temperature is NaN")
    eos = [int(e) for e in (eos_ids if eos_ids is not None else ())]
    if len(eos) > SAMPLE_MAX_EOS:
        raise ValueError(f"at most {SAMPLE_MAX_EOS} EOS ids, got {len(eos)}")
    if pad is None:
        pad = eos[0] if eos else 0
    p = _lib.AwqSampleParams()
    p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    p.do_sample = 1 if do_sample else 0
    p.temperature = temperature
    p.top_k = min(top_k, 0x7FFFFFFF)
    p.top_p = top_p
    p.n_eos = len(eos)
    p.pad = int(pad)
    for i, e in enumerate(eos):
        p.eos[i] = e
    return torch.frombuffer(bytearray(bytes(p)), dtype=torch.uint8)


def sample_proc_params(repetition_penalty=1.0, min_new_tokens=0):
    """Validate the logit processors and pack them as struct AwqSampleProc: a 16-byte CPU uint8 tensor the caller copies to the
    device.  repetition_penalty finite and > 0 (1 = off), min_new_tokens >= 0 (0 = off) -- transformers' checks."""
    p = float(repetition_penalty)
    if not math.isfinite(p) or p <= 0.0:
        raise ValueError(f"repetition_penalty has to be a strictly positive float, got {repetition_penalty}")
    if isinstance(min_new_tokens, bool) or int(min_new_tokens) != min_new_tokens or int(min_new_tokens) < 0:
        raise ValueError(f"min_new_tokens has to be a non-negative integer, got {min_new_tokens}")
    q = _lib.AwqSampleProc()
    q.repetition_penalty = p
    q.min_new_tokens = min(int(min_new_tokens), 0x7FFFFFFF)
    return torch.frombuffer(bytearray(bytes(q)), dtype=torch.uint8)


def sample_history_words(vocab):
    """int32 words per row of a sampler history: bit v % 32 of word v / 32 = token v seen"""
    return (int(vocab) + 31) // 32


def sample_history(ids, vocab, out=None):
    """OR the ids [B, S] (or [S]: one row; int64, on the device) into a history: int32 [B, >= ceil(vocab / 32)] on the device,
    bit v % 32 of word v / 32 set for every id v of row b.  out=None: a new zeroed history; otherwise `out` is extended in place
    (its earlier bits stay).  Ids outside [0, vocab) are refused (this waits for the device once to check them)."""
    V = int(vocab)
    if not 1 <= V <= 1 << 20:
        raise ValueError(f"sample_history: vocab must be in [1, 2^20], got {vocab}")
    if not isinstance(ids, torch.Tensor) or ids.dim() not in (1, 2) or ids.dtype not in (torch.int64, torch.int32):
        raise ValueError("sample_history: ids must be an int64 [B, S] tensor")
    ids2 = ids.view(1, -1) if ids.dim() == 1 else ids
    B, S = ids2.shape
    if ids2.numel() and bool(((ids2 < 0) | (ids2 >= V)).any()):
        raise ValueError(f"sample_history: ids outside [0, {V})")
    if out is None:
        _require_gpu(ids2)
        with torch.inference_mode(False):
            out = torch.zeros((B, sample_history_words(V)), dtype=torch.int32, device=ids2.device)
    if out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < sample_history_words(V) or out.stride(1) != 1:
        raise ValueError(f"sample_history: out must be int32 [{B}, >= {sample_history_words(V)}] with unit column stride")
    _require_gpu(ids2, out)
    if B == 0 or S == 0:
        return out
    ids2 = ids2.long()
    if ids2.stride(1) != 1:
        ids2 = ids2.contiguous()
    with torch.cuda.device(out.device):
        rc = _lib.lib().awq_sample_history_seed(_ptr(out), out.stride(0), _ptr(ids2), ids2.stride(0), B, S, V, _stream())
    _lib.check(rc, "awq_sample_history_seed")
    return out


def sample_workspace_bytes(B, V):
    return int(_lib.lib().awq_sample_workspace_bytes(B, V))


def _sample_workspace(device, nbytes):
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    ws = _sample_workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _retired_raw.append(ws)  # a captured graph may still hold it
        with torch.inference_mode(False):
            ws = torch.zeros(max(int(nbytes), 1 << 16), dtype=torch.uint8, device=device)
        _sample_workspaces[key] = ws
    return ws


def _logits_rows(logits, fn="sample_tokens"):
    """[B, V] or [B, T, V] (the last position) fp16 with unit element stride -> (view [B, V], row stride)."""
    if logits.dtype != torch.float16 or logits.dim() not in (2, 3):
        raise _lib.AwqHipError(f"{fn}: fp16 logits [B, V] or [B, T, V] expected, got {logits.dtype} {tuple(logits.shape)}")
    rows = logits[:, -1, :] if logits.dim() == 3 else logits
    if rows.stride(1) != 1:
        rows = rows.contiguous()
    return rows, rows.stride(0)


def _sample_launch_args(fn, a, logits, params, t, out, status, workspace, ring, finished, greedy, proc, history, max_new=None,
                        per_row=False):
    """What sample_launch and sample_launch_rows share: the checks of the buffers both forms take, in the order they always
    had (messages prefixed with `fn`; per_row: params and proc hold one struct per row), and the fields their argument structs
    have in common.  Returns (the logits' rows, B)."""
    rows, rs = _logits_rows(logits)
    B, V = rows.shape
    _require_gpu(rows, params, t, out, status, workspace, ring, finished, proc, history, max_new)
    if (proc is None) != (history is None):
        raise _lib.AwqHipError(f"{fn}: proc and history go together")
    if history is not None and (history.dtype != torch.int32 or history.dim() != 2 or history.shape[0] != B
                                or history.shape[1] < sample_history_words(V) or history.stride(1) != 1):
        raise _lib.AwqHipError(f"{fn}: history must be int32 [{B}, >= {sample_history_words(V)}] with unit column stride")
    if per_row:
        if not params.is_contiguous() or params.numel() * params.element_size() < B * ctypes.sizeof(_lib.AwqSampleParams):
            raise _lib.AwqHipError(f"{fn}: params must hold {B} x 64 contiguous bytes (sample_params_rows)")
        if proc is not None and (not proc.is_contiguous() or proc.numel() * proc.element_size() < B * ctypes.sizeof(_lib.AwqSampleProc)):
            raise _lib.AwqHipError(f"{fn}: proc must hold {B} x 16 contiguous bytes (sample_proc_params_rows)")
    elif proc is not None and (proc.numel() * proc.element_size() < ctypes.sizeof(_lib.AwqSampleProc)):
        raise _lib.AwqHipError(f"{fn}: proc must hold 16 bytes (sample_proc_params)")
    if out.numel() < B or status.numel() * 32 < B or (finished is not None and finished.numel() < B):
        raise _lib.AwqHipError(f"{fn}: out / status / finished too small for the batch")
    if ring is not None and (ring.dim() != 2 or ring.shape[0] != B or not ring.is_contiguous() or ring.dtype != torch.int32):
        raise _lib.AwqHipError(f"{fn}: ring must be a contiguous int32 [B, cap] tensor")
    a.struct_bytes = ctypes.sizeof(a)
    a.flags = SAMPLE_FLAG_GREEDY if greedy else 0
    a.logits, a.B, a.V, a.row_stride = _ptr(rows), B, V, rs
    a.params, a.t = _ptr(params), _ptr(t)
    a.out, a.out_stride = _ptr(out), out.stride(0) if out.dim() else 1
    a.ring, a.ring_cap = _ptr(ring), ring.shape[1] if ring is not None else 0
    a.finished, a.status = _ptr(finished), _ptr(status)
    a.workspace, a.workspace_bytes = _ptr(workspace), workspace.numel()
    return rows, B


def sample_launch(logits, params, t, out, status, workspace, ring=None, finished=None, greedy=False, proc=None, history=None):
    """The raw launch (no validation of the configuration, no sync): every buffer a device tensor the caller owns --
    params (64 bytes, sample_params), t (int32 [1]), out (int64, one element per row, any row stride), status (int32,
    ceil(B / 32) words), workspace (zeroed once), ring (int32 [B, cap]) and finished (int32 [B]) optional.  proc (16 bytes,
    sample_proc_params) with history (int32 [B, >= ceil(V / 32)], sample_history): the logit processors, and the emitted
    tokens ORed into the history (awq_sample_tokens_ex).  Capturable."""
    a = _lib.AwqSampleArgs()
    rows, B = _sample_launch_args("sample_launch", a, logits, params, t, out, status, workspace, ring, finished, greedy, proc,
                                  history)
    if out.dtype != torch.int64 or t.dtype != torch.int32 or (finished is not None and finished.dtype != torch.int32):
        raise _lib.AwqHipError("sample_launch: out int64, t and finished int32 expected")
    with torch.cuda.device(rows.device):
        a.stream = _stream()
        if proc is None:
            rc = _lib.lib().awq_sample_tokens(ctypes.byref(a))
        else:
            q = _lib.AwqSampleProcArgs()
            q.struct_bytes = ctypes.sizeof(_lib.AwqSampleProcArgs)
            q.flags = 0
            q.proc, q.history, q.history_stride = _ptr(proc), _ptr(history), history.stride(0)
            rc = _lib.lib().awq_sample_tokens_ex(ctypes.byref(a), ctypes.byref(q))
    _lib.check(rc, "awq_sample_tokens" if proc is None else "awq_sample_tokens_ex")
    return out


def _sample_tokens(fn, launch, logits, params, proc, use_proc, t, greedy, out, ring, finished, status, history, max_new=None):
    """What sample_tokens and sample_tokens_rows share once the configuration is checked and packed (params, proc: CPU bytes; t: a
    device tensor or a list of ints; max_new: the rows form's list of budgets): the parameters to the device, out / status /
    workspace / history, the launch and, with a status of its own, the bad-row report."""
    rows, _ = _logits_rows(logits)
    _require_gpu(rows)
    B, V = rows.shape
    dev = rows.device
    need = sample_workspace_bytes(B, V)
    if need == 0:
        err = _lib.AwqHipError(f"{fn}: no kernel for B = {B}, V = {V} (limits B <= 1024, V <= 2^20)")
        err.code = _lib.ERR_UNSUPPORTED
        raise err
    with torch.cuda.device(dev):
        params_d = params.to(dev, non_blocking=False)
        t_d = t if isinstance(t, torch.Tensor) else torch.tensor(t, dtype=torch.int32, device=dev)
        if out is None:
            out = torch.empty(B, dtype=torch.int64, device=dev)
        own_status = status is None
        if own_status:
            status = torch.zeros((B + 31) // 32, dtype=torch.int32, device=dev)
        ws = _sample_workspace(dev, need)
        proc_d = hist = None
        if use_proc:
            proc_d = proc.to(dev, non_blocking=False)
            hist = history if history is not None else torch.zeros((B, sample_history_words(V)), dtype=torch.int32, device=dev)
        more = {} if max_new is None else {"max_new": torch.tensor(max_new, dtype=torch.int32, device=dev)}
        launch(rows, params_d, t_d, out, status, ws, ring=ring, finished=finished, greedy=greedy, proc=proc_d, history=hist, **more)
        if own_status:
            bad = [r for r in range(B) if (int(status[r // 32].item()) >> (r % 32)) & 1] if bool(status.any()) else []
            if bad:
                raise _lib.AwqHipError(f"{fn}: rows {bad} hold NaN / +inf logits or keep no token (emitted pad)")
    return out


def sample_tokens(logits, *, do_sample, temperature=1.0, top_k=0, top_p=1.0, seed=0, t=1, eos_ids=(), pad=None, out=None,
                  ring=None, finished=None, status=None, repetition_penalty=1.0, min_new_tokens=0, history=None):
    """One token per row of fp16 logits [B, V] (or the last position of [B, T, V]), chosen on the device by
    csrc/sample.hip: greedy argmax (ties to the lowest index), or temperature -> top-k -> top-p -> Gumbel-max draw with
    Philox4x64-10 numbers keyed by (seed, t, row).  t is the 1-based index of the generated token (an int, or an int32 [1]
    device word the launch advances by one).  Returns out (int64 [B]).  ring (int32 [B, cap]) receives the token at column
    t - 1; finished (int32 [B]) latches on an EOS id, after which the row emits pad.  Without `status` the call waits for
    the result and raises AwqHipError if a row held NaN / +inf or kept nothing; with an int32 status tensor the bits are
    left there (sticky) and the call does not synchronise.
    Logit processors (transformers' order, before the warpers, greedy too): while t <= min_new_tokens the EOS ids are -inf;
    logits of the ids set in `history` (int32 [B, >= ceil(V / 32)], sample_history) are divided by repetition_penalty (positive
    ones) or multiplied by it (negative ones), then rounded to fp16.  With a history the emitted tokens are ORed into it in
    place, so a loop of calls behaves like transformers' `input_ids`.  A penalty other than 1 needs a history."""
    proc = sample_proc_params(repetition_penalty, min_new_tokens)
    if float(repetition_penalty) != 1.0 and history is None:
        raise ValueError("sample_tokens: repetition_penalty needs a history of the ids seen (sample_history)")
    use_proc = history is not None or int(min_new_tokens) > 0
    params = sample_params(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, eos_ids=eos_ids,
                           pad=pad)
    if not isinstance(t, torch.Tensor) and int(t) < 1:
        raise ValueError(f"t is the 1-based token index, got {t}")
    return _sample_tokens("sample_tokens", sample_launch, logits, params, proc, use_proc, t if isinstance(t, torch.Tensor) else [int(t)],
                          not do_sample or temperature <= 0, out, ring, finished, status, history)


# ---- the sampler's rows form: per-row parameters and token indices (awq_sample_tokens_rows) ------------------------------------

def is_seq(v):
    if isinstance(v, torch.Tensor):
        return v.dim() > 0
    return hasattr(v, "__len__") and not isinstance(v, (str, bytes))


def per_row(name, value, B):
    """A per-row argument as a list of B values: a scalar is broadcast, a sequence (list, tuple, array, tensor) must hold B."""
    if not is_seq(value):
        return [value.item() if isinstance(value, torch.Tensor) else value] * B
    vals = value.tolist() if hasattr(value, "tolist") else list(value)
    if len(vals) != B:
        raise ValueError(f"{name}: a sequence of {len(vals)} values for {B} rows")
    return vals


def _eos_rows(eos_ids, B):
    """one tuple of ids for every row, or one tuple (or None) per row"""
    if eos_ids is None:
        return [()] * B
    if not is_seq(eos_ids):
        return [(int(eos_ids),)] * B
    eos = list(eos_ids)
    if not any(e is None or is_seq(e) for e in eos):
        return [tuple(eos)] * B
    if len(eos) != B:
        raise ValueError(f"eos_ids: {len(eos)} per-row lists for {B} rows")
    return [() if e is None else tuple(e) if is_seq(e) else (int(e),) for e in eos]


def sample_params_rows(B, *, do_sample, temperature=1.0, top_k=0, top_p=1.0, seed=0, eos_ids=(), pad=None):
    """sample_params for B rows: struct AwqSampleParams [B] as a CPU uint8 [B, 64] tensor the caller copies to the device.  Each
    argument is a scalar (broadcast) or a sequence of B values; eos_ids one tuple, or one tuple per row; pad defaults per row
    to the row's first EOS id.  The checks are sample_params'; a ValueError names the offending row.  Host only."""
    B = int(B)
    if B < 1:
        raise ValueError(f"sample_params_rows: B must be >= 1, got {B}")
    cols = {k: per_row(k, v, B) for k, v in (("do_sample", do_sample), ("temperature", temperature), ("top_k", top_k),
                                              ("top_p", top_p), ("seed", seed), ("pad", pad))}
    eos = _eos_rows(eos_ids, B)
    out = torch.empty((B, ctypes.sizeof(_lib.AwqSampleParams)), dtype=torch.uint8)
    for r in range(B):
        try:
            out[r] = sample_params(eos_ids=eos[r], **{k: v[r] for k, v in cols.items()})
        except (ValueError, TypeError) as e:
            raise ValueError(f"row {r}: {e}") from None
    return out


def sample_proc_params_rows(B, repetition_penalty=1.0, min_new_tokens=0):
    """sample_proc_params for B rows: struct AwqSampleProc [B] as a CPU uint8 [B, 16] tensor; scalars are broadcast.  A
    ValueError names the offending row.  Host only."""
    B = int(B)
    if B < 1:
        raise ValueError(f"sample_proc_params_rows: B must be >= 1, got {B}")
    pen, mn = per_row("repetition_penalty", repetition_penalty, B), per_row("min_new_tokens", min_new_tokens, B)
    out = torch.empty((B, ctypes.sizeof(_lib.AwqSampleProc)), dtype=torch.uint8)
    for r in range(B):
        try:
            out[r] = sample_proc_params(pen[r], mn[r])
        except (ValueError, TypeError) as e:
            raise ValueError(f"row {r}: {e}") from None
    return out


def sample_launch_rows(logits, params, t, out, status, workspace, ring=None, finished=None, greedy=False, proc=None, history=None,
                       max_new=None):
    """sample_launch with every row a request of its own (awq_sample_tokens_rows): params (uint8 [B, 64], sample_params_rows)
    and t (int32 [B], advanced per row by the launch) are read per row; proc (uint8 [B, 16], sample_proc_params_rows) with
    history as in sample_launch; max_new (int32 [B], with finished): row r latches finished[r] in the launch that emits its
    token index max_new[r] (<= 0: no limit).  greedy: argmax for every row in one launch.  No validation of the configuration,
    no sync.  Capturable."""
    a = _lib.AwqSampleRowsArgs()
    rows, B = _sample_launch_args("sample_launch_rows", a, logits, params, t, out, status, workspace, ring, finished, greedy, proc,
                                  history, max_new, per_row=True)
    if out.dtype != torch.int64 or (finished is not None and finished.dtype != torch.int32):
        raise _lib.AwqHipError("sample_launch_rows: out int64 and finished int32 expected")
    for name, w in (("t", t), ("max_new", max_new)):
        if w is not None and (w.dtype != torch.int32 or w.numel() < B or not w.is_contiguous()):
            raise _lib.AwqHipError(f"sample_launch_rows: {name} must be a contiguous int32 [{B}] tensor")
    if max_new is not None and finished is None:
        raise _lib.AwqHipError("sample_launch_rows: max_new latches `finished`: pass both")
    a.proc, a.history, a.history_stride = _ptr(proc), _ptr(history), history.stride(0) if history is not None else 0
    a.max_new = _ptr(max_new)
    with torch.cuda.device(rows.device):
        a.stream = _stream()
        rc = _lib.lib().awq_sample_tokens_rows(ctypes.byref(a))
    _lib.check(rc, "awq_sample_tokens_rows")
    return out


def sample_tokens_rows(logits, *, do_sample, temperature=1.0, top_k=0, top_p=1.0, seed=0, t=1, eos_ids=(), pad=None, out=None,
                       ring=None, finished=None, status=None, repetition_penalty=1.0, min_new_tokens=0, history=None,
                       max_new_tokens=None):
    """sample_tokens with every row a request of its own: each of do_sample, temperature, top_k, top_p, seed, pad,
    repetition_penalty, min_new_tokens and max_new_tokens is a scalar (broadcast) or a sequence of B values, eos_ids one tuple or
    one tuple per row, and t -- the 1-based index of the token each row generates -- an int, a sequence of B ints, or an int32 [B]
    device tensor that the launch advances per row.  Row r's token is row r of sample_tokens on the same logits with row r's
    values and t = t[r].  max_new_tokens (with `finished`): row r latches finished[r] with the token of index max_new_tokens[r].
    Returns out (int64 [B]).  Status handling, history and the processors as in sample_tokens.  The loop of one's own over
    slots that are refilled one by one: keep t, finished and history on the device and rewrite a slot's words when it takes a
    new request."""
    rows, _ = _logits_rows(logits)
    B, V = rows.shape
    params = sample_params_rows(B, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                eos_ids=eos_ids, pad=pad)
    proc = sample_proc_params_rows(B, repetition_penalty, min_new_tokens)
    pens, mins = per_row("repetition_penalty", repetition_penalty, B), per_row("min_new_tokens", min_new_tokens, B)
    if any(float(p) != 1.0 for p in pens) and history is None:
        raise ValueError("sample_tokens_rows: repetition_penalty needs a history of the ids seen (sample_history)")
    use_proc = history is not None or any(int(m) > 0 for m in mins)
    if not isinstance(t, torch.Tensor):
        t = [int(v) for v in per_row("t", t, B)]
        for r, v in enumerate(t):
            if v < 1:
                raise ValueError(f"row {r}: t is the 1-based token index, got {v}")
    max_rows = None
    if max_new_tokens is not None:
        max_rows = [int(m) for m in per_row("max_new_tokens", max_new_tokens, B)]
        if finished is None:
            raise ValueError("sample_tokens_rows: max_new_tokens latches `finished`: pass a finished tensor")
    ds, temps = per_row("do_sample", do_sample, B), per_row("temperature", temperature, B)
    greedy = all(not d or float(T) <= 0 for d, T in zip(ds, temps))
    return _sample_tokens("sample_tokens_rows", sample_launch_rows, rows, params, proc, use_proc, t, greedy, out, ring, finished, status,
                          history, max_new=max_rows)


# ---- the sampler over the slots of a verify step (awq_sample_tokens_slots) --------------------------------------------------------

def sample_launch_slots(logits, params, cnt, tok, pred, status, workspace, finished=None, greedy=False, proc=None, history=None):
    """The raw launch of awq_sample_tokens_slots (no validation of the configuration, no sync): logits fp16 [B, T, V] or
    [B * T, V], row b * T + j the slot j of request b; params (uint8 [B, 64], sample_params_rows), cnt (int32 [B]: tokens generated
    so far), tok (int64 [B, T]: the step's input -- the last token, then the drafts), pred (int64 [B * T]: the slots' tokens),
    status (int32, ceil(B * T / 32) words), workspace (sample_workspace_bytes(B * T, V), zeroed once), finished (int32 [B],
    optional); proc (uint8 [B, 16]) with history (int32 [B, >= ceil(V / 32)]).  Slot (b, j) gets the token the rows form emits for
    request b at token index cnt[b] + 1 + j with tok[b, 1 .. j] added to the seen ids.  Only pred and status are written.
    Capturable."""
    fn = "sample_launch_slots"
    if tok is None or tok.dim() != 2 or tok.dtype != torch.int64 or not tok.is_contiguous():
        raise _lib.AwqHipError(f"{fn}: tok must be a contiguous int64 [B, T] tensor")
    B, T = tok.shape
    if logits.dtype != torch.float16 or logits.dim() not in (2, 3):
        raise _lib.AwqHipError(f"{fn}: fp16 logits [B, T, V] or [B * T, V] expected, got {logits.dtype} {tuple(logits.shape)}")
    rows = logits.reshape(-1, logits.shape[-1]) if logits.dim() == 3 else logits
    if rows.stride(1) != 1:
        rows = rows.contiguous()
    if rows.shape[0] != B * T:
        raise _lib.AwqHipError(f"{fn}: {rows.shape[0]} logits rows for {B} x {T} slots")
    V = rows.shape[1]
    _require_gpu(rows, params, cnt, tok, pred, status, workspace, finished, proc, history)
    if (proc is None) != (history is None):
        raise _lib.AwqHipError(f"{fn}: proc and history go together")
    if history is not None and (history.dtype != torch.int32 or history.dim() != 2 or history.shape[0] != B
                                or history.shape[1] < sample_history_words(V) or history.stride(1) != 1):
        raise _lib.AwqHipError(f"{fn}: history must be int32 [{B}, >= {sample_history_words(V)}] with unit column stride")
    if not params.is_contiguous() or params.numel() * params.element_size() < B * ctypes.sizeof(_lib.AwqSampleParams):
        raise _lib.AwqHipError(f"{fn}: params must hold {B} x 64 contiguous bytes (sample_params_rows)")
    if proc is not None and (not proc.is_contiguous() or proc.numel() * proc.element_size() < B * ctypes.sizeof(_lib.AwqSampleProc)):
        raise _lib.AwqHipError(f"{fn}: proc must hold {B} x 16 contiguous bytes (sample_proc_params_rows)")
    if pred.dtype != torch.int64 or pred.numel() < B * T or not pred.is_contiguous():
        raise _lib.AwqHipError(f"{fn}: pred must be a contiguous int64 tensor of B * T elements")
    if status.dtype != torch.int32 or status.numel() * 32 < B * T:
        raise _lib.AwqHipError(f"{fn}: status must hold one bit per (row, slot)")
    for name, w in (("cnt", cnt), ("finished", finished)):
        if w is not None and (w.dtype != torch.int32 or w.numel() < B or not w.is_contiguous()):
            raise _lib.AwqHipError(f"{fn}: {name} must be a contiguous int32 [{B}] tensor")
    a = _lib.AwqSampleSlotsArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.flags = SAMPLE_FLAG_GREEDY if greedy else 0
    a.logits, a.B, a.T, a.V, a.row_stride = _ptr(rows), B, T, V, rows.stride(0)
    a.params, a.cnt, a.tok, a.pred = _ptr(params), _ptr(cnt), _ptr(tok), _ptr(pred)
    a.finished, a.status = _ptr(finished), _ptr(status)
    a.workspace, a.workspace_bytes = _ptr(workspace), workspace.numel()
    a.proc, a.history, a.history_stride = _ptr(proc), _ptr(history), history.stride(0) if history is not None else 0
    with torch.cuda.device(rows.device):
        a.stream = _stream()
        rc = _lib.lib().awq_sample_tokens_slots(ctypes.byref(a))
    _lib.check(rc, "awq_sample_tokens_slots")
    return pred


def sample_tokens_slots(logits, tok, cnt, *, do_sample, temperature=1.0, top_k=0, top_p=1.0, seed=0, eos_ids=(), pad=None,
                        repetition_penalty=1.0, min_new_tokens=0, history=None, finished=None, status=None, greedy=False):
    """The tokens of the B x T slots of a verify step (see sample_launch_slots): logits fp16 [B, T, V], tok int64 [B, T] and cnt
    int32 [B] on the device; the sampling arguments and processors per request as in sample_tokens_rows (a scalar, or a sequence
    of B values).  Returns pred int64 [B, T]: slot (b, j) is the token sample_tokens_rows emits for request b at t = cnt[b] + 1 + j
    with the drafts tok[b, 1 .. j] added to its history.  Nothing but the result (and `status`) is written.  Without `status` the
    call waits for the result and raises AwqHipError if a slot held NaN / +inf or kept nothing.  greedy: force the argmax."""
    if tok.dim() != 2:
        raise ValueError("sample_tokens_slots: tok must be [B, T]")
    B, T = tok.shape
    params = sample_params_rows(B, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                eos_ids=eos_ids, pad=pad)
    proc = sample_proc_params_rows(B, repetition_penalty, min_new_tokens)
    pens, mins = per_row("repetition_penalty", repetition_penalty, B), per_row("min_new_tokens", min_new_tokens, B)
    if any(float(p) != 1.0 for p in pens) and history is None:
        raise ValueError("sample_tokens_slots: repetition_penalty needs a history of the ids seen (sample_history)")
    use_proc = history is not None or any(int(m) > 0 for m in mins)
    _require_gpu(logits, tok, cnt)
    V, dev = logits.shape[-1], logits.device
    need = sample_workspace_bytes(B * T, V)
    if need == 0:
        err = _lib.AwqHipError(f"sample_tokens_slots: no kernel for B * T = {B * T}, V = {V} (limits B * T <= 1024, V <= 2^20)")
        err.code = _lib.ERR_UNSUPPORTED
        raise err
    with torch.cuda.device(dev):
        pred = torch.empty(B * T, dtype=torch.int64, device=dev)
        own_status = status is None
        if own_status:
            status = torch.zeros((B * T + 31) // 32, dtype=torch.int32, device=dev)
        proc_d = hist = None
        if use_proc:
            proc_d = proc.to(dev)
            hist = history if history is not None else torch.zeros((B, sample_history_words(V)), dtype=torch.int32, device=dev)
        sample_launch_slots(logits, params.to(dev), cnt, tok, pred, status, _sample_workspace(dev, need), finished=finished,
                            greedy=greedy, proc=proc_d, history=hist)
        if own_status and bool(status.any()):
            st = status.cpu().tolist()
            bad = [(r // T, r % T) for r in range(B * T) if (st[r // 32] >> (r % 32)) & 1]
            raise _lib.AwqHipError(f"sample_tokens_slots: slots {bad} hold NaN / +inf logits or keep no token (emitted pad)")
    return pred.view(B, T)


# ---- speculative decoding: the verify step's attention (csrc/verify_attn.hip), acceptance and prompt-lookup drafts (csrc/spec.hip)

_verify_workspaces = {}


def verify_attention_splits(max_len, B, T, n_heads, n_kv_heads):
    """split count of a verify_attention_rows launch sized for max_len (host only; the tests' error bound reads it)"""
    rc = int(_lib.lib().awq_verify_attention_splits(int(max_len), int(B), int(T), int(n_heads), int(n_kv_heads)))
    if rc < 1:
        _lib.check(rc, "awq_verify_attention_splits")
    return rc


def verify_attention_rows(q, k_cache, v_cache, pos_rows, max_len=None, scale=None, k_scale=None, v_scale=None):
    """q [B, T, Hq, 128] fp16 -- the q_out of rope_kv_append(pos_rows=..., S = T), which has already written cache rows
    pos_rows[b] .. pos_rows[b] + T - 1 -- caches [>= B, Tmax, Hkv, 128] fp16, pos_rows int32 [B] on the device: the position of
    sequence b's FIRST new token.  Returns [B, T, Hq, 128]: query (b, j) attends over cache rows t <= pos_rows[b] + j
    (awq_verify_attention_rows).  T in 2 .. 8; max_len (default: the cache window) is the host bound of pos_rows[b] + T the
    launch is sized for.  An fp8 cache is refused (NotImplementedError)."""
    if k_scale is not None or v_scale is not None or k_cache.dtype == torch.uint8:
        raise NotImplementedError('verify_attention_rows: kv_cache_dtype="fp8" is not supported by the speculative path')
    _require_gpu(q, k_cache, v_cache, pos_rows)
    if q.dtype != torch.float16 or k_cache.dtype != torch.float16 or v_cache.dtype != torch.float16 or q.dim() != 4:
        raise _lib.AwqHipError("verify_attention_rows expects fp16 q [B, T, Hq, D] and fp16 caches")
    B, T, Hq, D = q.shape
    Tmax, Hkv = k_cache.shape[1], k_cache.shape[2]
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()) or k_cache.shape[0] < B or k_cache.shape != v_cache.shape:
        raise _lib.AwqHipError("verify_attention_rows: caches must be contiguous [>=B, Tmax, Hkv, D]")
    _check_rows("verify_attention_rows", "pos", pos_rows, None, B, q.device)
    q = q.contiguous()
    out = torch.empty_like(q)
    L = _lib.lib()
    ws = _stream_workspace(_verify_workspaces, q.device, max(L.awq_verify_attention_workspace_bytes(B, T, Hq), 16))
    if scale is None:
        scale = D ** -0.5
    with torch.cuda.device(q.device):
        _lib.check(L.awq_verify_attention_rows(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), _ptr(pos_rows),
                                               int(max_len if max_len is not None else Tmax), B, T, Hq, Hkv, D, Tmax, float(scale),
                                               _ptr(ws), ws.numel(), _stream()), "awq_verify_attention_rows")
    return out


def spec_params(eos_ids=(), pad=0, max_new_tokens=1, ngram_max=3):
    """struct AwqSpecParams as a 48-byte CPU uint8 tensor the caller copies to the device"""
    eos = [int(e) for e in eos_ids]
    if len(eos) > 8:
        raise ValueError("at most 8 EOS ids")
    if int(ngram_max) < 1 or int(ngram_max) > 8:
        raise ValueError(f"draft_ngram must be in 1 .. 8, got {ngram_max}")
    p = _lib.AwqSpecParams()
    p.n_eos, p.pad, p.max_new_tokens, p.ngram_max = len(eos), int(pad), int(max_new_tokens), int(ngram_max)
    for i, e in enumerate(eos):
        p.eos[i] = e
    return torch.frombuffer(bytearray(bytes(p)), dtype=torch.uint8)


def _spec_args(params, tok, hist, n_hist, pred=None, cnt=None, ring=None, finished=None, pos_rows=None, len_rows=None, status=None,
               steps=None):
    _require_gpu(params, tok, hist, n_hist, pred, cnt, ring, finished, pos_rows, len_rows, status, steps)
    if tok.dtype != torch.int64 or tok.dim() != 2 or not tok.is_contiguous():
        raise _lib.AwqHipError("spec: tok must be a contiguous int64 [B, T] tensor")
    B, T = tok.shape
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] != B or not hist.is_contiguous():
        raise _lib.AwqHipError("spec: hist must be a contiguous int32 [B, cap] tensor")
    if params.numel() * params.element_size() < ctypes.sizeof(_lib.AwqSpecParams):
        raise _lib.AwqHipError("spec: params must hold 48 bytes (spec_params)")
    words = [("n_hist", n_hist), ("cnt", cnt), ("finished", finished), ("pos_rows", pos_rows), ("len_rows", len_rows),
             ("steps", steps)]
    for name, x in words:
        if x is not None and (x.dtype != torch.int32 or x.numel() < B or not x.is_contiguous()):
            raise _lib.AwqHipError(f"spec: {name} must be a contiguous int32 [B] tensor")
    if ring is not None and (ring.dtype != torch.int32 or ring.dim() != 2 or ring.shape[0] != B or not ring.is_contiguous()):
        raise _lib.AwqHipError("spec: ring must be a contiguous int32 [B, cap] tensor")
    if pred is not None and (pred.dtype != torch.int64 or pred.numel() < B * T or not pred.is_contiguous()):
        raise _lib.AwqHipError("spec: pred must be a contiguous int64 tensor of B * T elements")
    if status is not None and (status.dtype != torch.int32 or status.numel() * 32 < B * T):
        raise _lib.AwqHipError("spec: status must hold one bit per (row, slot)")
    a = _lib.AwqSpecArgs()
    a.struct_bytes, a.flags, a.B, a.T = ctypes.sizeof(_lib.AwqSpecArgs), 0, B, T
    a.params, a.tok, a.pred = _ptr(params), _ptr(tok), _ptr(pred)
    a.hist, a.hist_cap, a.n_hist, a.cnt = _ptr(hist), hist.shape[1], _ptr(n_hist), _ptr(cnt)
    a.ring, a.ring_cap = _ptr(ring), ring.shape[1] if ring is not None else 0
    a.finished, a.pos_rows, a.len_rows, a.status = _ptr(finished), _ptr(pos_rows), _ptr(len_rows), _ptr(status)
    a.steps = _ptr(steps)
    return a


def spec_accept(params, tok, pred, hist, n_hist, cnt, ring, finished, pos_rows, len_rows, status=None, steps=None, history=None,
                vocab=None):
    """awq_spec_accept on device words the caller owns (include/awq_hip.h states the rule; tests/spec_ref.py restates it).
    history (int32 [B, >= ceil(vocab / 32)], with vocab): awq_spec_accept_ex -- the bit of every emitted token is set in the
    sampler's penalty history of its row.  Capturable, no sync."""
    a = _spec_args(params, tok, hist, n_hist, pred, cnt, ring, finished, pos_rows, len_rows, status, steps)
    if history is None:
        with torch.cuda.device(tok.device):
            a.stream = _stream()
            _lib.check(_lib.lib().awq_spec_accept(ctypes.byref(a)), "awq_spec_accept")
        return
    if vocab is None:
        raise _lib.AwqHipError("spec_accept: history needs vocab")
    _require_gpu(history)
    if (history.dtype != torch.int32 or history.dim() != 2 or history.shape[0] != tok.shape[0]
            or history.shape[1] < sample_history_words(vocab) or history.stride(1) != 1):
        raise _lib.AwqHipError(f"spec_accept: history must be int32 [{tok.shape[0]}, >= {sample_history_words(vocab)}] with unit "
                               "column stride")
    q = _lib.AwqSpecHistoryArgs()
    q.struct_bytes, q.flags = ctypes.sizeof(q), 0
    q.history, q.history_stride, q.V = _ptr(history), history.stride(0), int(vocab)
    with torch.cuda.device(tok.device):
        a.stream = _stream()
        _lib.check(_lib.lib().awq_spec_accept_ex(ctypes.byref(a), ctypes.byref(q)), "awq_spec_accept_ex")


def ngram_draft(params, tok, hist, n_hist):
    """awq_ngram_draft: tok [B, T] = each row's last token and its T - 1 prompt-lookup drafts.  Capturable, no sync."""
    a = _spec_args(params, tok, hist, n_hist)
    with torch.cuda.device(tok.device):
        a.stream = _stream()
        _lib.check(_lib.lib().awq_ngram_draft(ctypes.byref(a)), "awq_ngram_draft")


# ---- token log-probabilities (csrc/logprob.hip) ----------------------------------------------------------------------------------

def _logprob_call(rows, row_stride, R, V, ids, ids_stride, out, out_stride, slot, out_cap):
    a = _lib.AwqLogprobArgs()
    a.logits, a.logits_stride, a.ids, a.ids_stride = _ptr(rows), row_stride, _ptr(ids), ids_stride
    a.out, a.out_stride, a.slot, a.out_cap = _ptr(out), out_stride, _ptr(slot), out_cap
    a.R, a.V = R, V
    with torch.cuda.device(rows.device):
        a.stream = _stream()
        rc = _lib.lib().awq_token_logprobs(ctypes.byref(a))
    _lib.check(rc, "awq_token_logprobs")


def token_logprobs_launch(logits, ids, out, slot=None):
    """The raw launch (no validation beyond dtypes, no sync), on buffers the caller owns: logits fp16 [R, V] (or the last position
    of [R, T, V]), ids int64 with one element per row (any row stride), out fp32 [R] -- or, with slot (int32 [R]), out fp32
    [R, cap]: row r writes out[r, slot[r]] (dropped at slot[r] >= cap) and slot[r] += 1.  Capturable."""
    rows, rs = _logits_rows(logits, "token_logprobs_launch")
    _require_gpu(rows, ids, out, slot)
    if ids.dtype != torch.int64 or out.dtype != torch.float32 or (slot is not None and slot.dtype != torch.int32):
        raise _lib.AwqHipError("token_logprobs_launch: ids int64, out fp32 and slot int32 expected")
    R, V = rows.shape
    _logprob_call(rows, rs, R, V, ids, ids.stride(0) if ids.dim() else 1, out, out.stride(0) if out.dim() else 1, slot,
                  out.shape[1] if slot is not None and out.dim() == 2 else (1 if slot is not None else 0))
    return out


def token_logprobs(logits, ids, out=None):
    """log p(ids | logits) per row -> fp32 of ids' shape: (x[id] - max x) - log sum exp(x - max x) over the fp16 logits [..., V]
    cast to fp32 (csrc/logprob.hip, one block per row; no fp32 copy of the logits is made).  This is the model's own
    distribution: temperature, top-k / top-p and the logit processors are NOT applied -- what perplexity needs and what serving
    APIs return as `logprobs`.  ids int64 with the leading shape of logits; id < 0 marks an ignored slot (shifted labels, pads,
    masked positions) and gives 0.0; id >= V gives NaN, as does a row holding NaN or +inf or nothing but -inf; -inf logits are
    legal (the id's own: -inf).  The last dimension of logits must be contiguous; leading dimensions that do not collapse to one
    row stride are made contiguous once."""
    if not isinstance(logits, torch.Tensor) or not isinstance(ids, torch.Tensor):
        raise _lib.AwqHipError("token_logprobs: tensors expected")
    if logits.dtype != torch.float16 or logits.dim() < 1:
        raise _lib.AwqHipError(f"token_logprobs: fp16 logits [..., V] expected, got {logits.dtype} {tuple(logits.shape)}")
    if ids.dtype != torch.int64 or tuple(ids.shape) != tuple(logits.shape[:-1]):
        raise _lib.AwqHipError(f"token_logprobs: ids must be int64 {tuple(logits.shape[:-1])}, got {ids.dtype} {tuple(ids.shape)}")
    V = int(logits.shape[-1])
    if not 1 <= V <= 1 << 20:
        raise _lib.AwqHipError(f"token_logprobs: vocabulary {V} outside 1 .. 2^20")
    if V > 1 and logits.stride(-1) != 1:
        raise _lib.AwqHipError("token_logprobs: the last dimension of logits must be contiguous")
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != tuple(ids.shape) or not out.is_contiguous()):
        raise _lib.AwqHipError(f"token_logprobs: out must be contiguous fp32 {tuple(ids.shape)}")
    _require_gpu(logits, ids, out)
    lead = [(n, s) for n, s in zip(logits.shape[:-1], logits.stride()[:-1]) if n != 1]
    R = math.prod(logits.shape[:-1])
    if R > 0 and not all(so == ni * si for (_, so), (ni, si) in zip(lead, lead[1:])):
        logits, lead = logits.contiguous(), [(R, V)]
    stride = lead[-1][1] if lead else V
    if stride < V:  # (expanded rows and the like)
        logits, stride = logits.contiguous(), V
    if out is None:
        out = torch.empty(ids.shape, dtype=torch.float32, device=logits.device)
    if R:
        _logprob_call(logits, stride, R, V, ids.contiguous(), 1, out, 1, None, 0)
    return out
