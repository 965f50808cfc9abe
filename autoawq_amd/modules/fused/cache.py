"""KV store of the fused attention block for MI355X.

Role of `WindowedCache` (reference: awq/modules/fused/cache.py:4-79) with the same method surface --
`get_kv`, `update_kv`, `roll_kv_n_steps`, `to`, `increase_batch_size`, `decrease_batch_size`, attributes
`k`, `v`, `max_seq_len` -- but its own design:

  * ONE allocation `kv[2, batch, max_seq_len, kv_heads, head_dim]` fp16; `k` / `v` are views of it (the
    decode kernels take two base pointers, the sequence axis is dim 1 of each view: a cache row of one
    (token, head) is 256 contiguous bytes, what `awq_decode_attention` reads per lane group);
  * dropping the n oldest positions moves only the LIVE rows (`start_pos - n` of them) forward with one
    strided device copy through a scratch of exactly that size.  The reference rolls and zero-fills the
    whole buffer (two full-size copies per layer); rows at or past the new length are never read
    (`awq_decode_attention` stops at the length), so nothing is cleared;
  * batch-size changes keep the prefix of sequences that survive instead of discarding everything.

dtype="fp8" (opt-in): `kv` holds OCP e4m3 codes (uint8, same layout) and `scales[2, batch, max_seq_len, kv_heads]` fp32 one
power-of-two scale per row (format: include/awq_hip.h); `k_scale` / `v_scale` are views of it, and every move of rows moves
their scales with them.  `get_kv` returns dequantized fp16 copies, `update_kv` quantizes.  Rows cost 132 bytes instead of 256.
"""
import torch

DTYPES = ("fp16", "fp8")


class WindowedCache:
    def __init__(self, cache_batch_size, n_heads, n_kv_heads, head_dim, max_seq_len, device, dtype="fp16"):
        if dtype not in DTYPES:
            raise ValueError(f"WindowedCache: dtype must be one of {DTYPES}, got {dtype!r}")
        heads = n_kv_heads if n_kv_heads != 0 else n_heads
        self.max_seq_len = int(max_seq_len)
        self.dtype = dtype
        self._alloc(int(cache_batch_size), heads, int(head_dim), device)

    def _alloc(self, batch, heads, head_dim, device, keep=None, keep_scales=None):
        fp8 = self.dtype == "fp8"
        with torch.inference_mode(False):  # a persistent buffer written in place from any context: never an inference tensor
            kv = torch.zeros((2, batch, self.max_seq_len, heads, head_dim), dtype=torch.uint8 if fp8 else torch.float16,
                             device=device)
            scales = torch.zeros((2, batch, self.max_seq_len, heads), dtype=torch.float32, device=device) if fp8 else None
            if keep is not None:
                n = min(batch, keep.shape[1])
                kv[:, :n] = keep[:, :n].to(device)
                if fp8:
                    scales[:, :n] = keep_scales[:, :n].to(device)
        self.kv = kv
        self.k, self.v = kv[0], kv[1]
        self.scales = scales
        self.k_scale, self.v_scale = (scales[0], scales[1]) if fp8 else (None, None)

    def _realloc(self, batch, device):
        self._alloc(batch, self.kv.shape[3], self.kv.shape[4], device, keep=self.kv, keep_scales=self.scales)

    # ---- reference surface -------------------------------------------------------------------
    def get_kv(self, batch_size, start_pos, seqlen):
        end = start_pos + seqlen
        if self.dtype == "fp8":
            return _dequant(self.v, self.v_scale, batch_size, end), _dequant(self.k, self.k_scale, batch_size, end)
        return self.v[:batch_size, :end], self.k[:batch_size, :end]

    def update_kv(self, values_store, keys_store, batch_size, start_pos, seqlen):
        if self.dtype == "fp8":
            _quant(keys_store, self.k, self.k_scale, start_pos)
            _quant(values_store, self.v, self.v_scale, start_pos)
            return
        rows = slice(start_pos, start_pos + seqlen)
        self.k[:batch_size, rows].copy_(keys_store)
        self.v[:batch_size, rows].copy_(values_store)

    def roll_kv_n_steps(self, start_pos, n=100):
        """Forget the n oldest positions; returns the new start position (reference: cache.py:47-62)."""
        n = max(0, min(int(n), int(start_pos), self.max_seq_len))
        live = int(start_pos) - n
        if n and live > 0:
            for buf in (self.kv, self.scales):
                if buf is not None:
                    moved = buf[:, :, n:n + live].clone()  # source and destination overlap: go through a scratch
                    buf[:, :, :live].copy_(moved)
        return live

    def roll_rows(self, rows, n):
        """Forget the n oldest positions of the sequences `rows` only (the other sequences keep their contents): cache rows
        n .. max_seq_len - 1 of each move to 0 .. max_seq_len - n - 1.  The per-sequence form of roll_kv_n_steps for batches
        whose sequences have their own lengths (modules/fused/decode.py); the caller lowers those sequences' positions by n."""
        n = max(0, min(int(n), self.max_seq_len))
        rows = [int(r) for r in rows]
        if not n or not rows or n == self.max_seq_len:
            return
        idx = torch.tensor(rows, dtype=torch.long, device=self.kv.device)
        for buf in (self.kv, self.scales):
            if buf is not None:
                moved = buf[:, idx, n:].clone()  # [2, len(rows), max_seq_len - n, heads(, head_dim)]
                buf[:, idx, : self.max_seq_len - n] = moved

    def to(self, device):
        self._realloc(self.kv.shape[1], device)

    def increase_batch_size(self, to_bsz):
        self._realloc(int(to_bsz), self.kv.device)

    def decrease_batch_size(self, to_bsz):
        self._realloc(int(to_bsz), self.kv.device)


def _quant(x, codes, scales, start):
    """fp16 rows x [B, S, Hkv, D] -> codes / scales of cache rows [start, start + S): awq_kv_quant_fp8 on the GPU.  A cache that
    lives on the CPU (there is no kernel there) gets the same format from torch's e4m3 cast."""
    if codes.is_cuda:
        from ... import ops

        ops.kv_quant_fp8(x.to(torch.float16), codes, scales, start)
        return
    B, S = x.shape[0], x.shape[1]
    c, s = quantize_rows_fp8(x)
    codes[:B, start:start + S] = c
    scales[:B, start:start + S] = s


def _dequant(codes, scales, batch, n):
    if codes.is_cuda:
        from ... import ops

        return ops.kv_dequant_fp8(codes, scales, n, batch)
    return dequantize_rows_fp8(codes[:batch, :n], scales[:batch, :n])


def quantize_rows_fp8(x):
    """torch form of the fp8 row format (include/awq_hip.h) for CPU-resident caches: x [..., D] -> (uint8 codes [..., D],
    fp32 scales [...])."""
    x = x.to(torch.float16).float()
    amax = x.abs().amax(dim=-1)
    bits = amax.view(torch.int32)
    k = (bits >> 23) - 127 - 8 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    finite = torch.isfinite(x).all(dim=-1)
    live = finite & (amax > 0)
    k = torch.where(live, k, torch.zeros_like(k))
    scale = ((127 + k) << 23).view(torch.float32)  # 2^k and 2^-k built from their bits: exact on every device
    inv = ((127 - k) << 23).view(torch.float32)
    y = torch.where(live[..., None], x * inv[..., None], torch.zeros_like(x))
    codes = y.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    scale = torch.where(live, scale, torch.where(finite, torch.zeros_like(scale), torch.full_like(scale, float("nan"))))
    return codes, scale


def dequantize_rows_fp8(codes, scales):
    v = codes.view(torch.float8_e4m3fn).float() * scales[..., None]
    return torch.where(v.abs() > 65504.0, torch.copysign(torch.full_like(v, 65504.0), v), v).to(torch.float16)
