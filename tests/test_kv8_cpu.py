"""fp8 KV cache, host side: the numpy restatement against torch's e4m3fn, WindowedCache("fp8") moves, argument validation and
the new C ABI symbols."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kv8_ref as ref


def _torch_codes(x, s):
    y = torch.from_numpy(np.clip(np.asarray(x, np.float64) / s[..., None], -448.0, 448.0))
    return y.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_decode_table_is_e4m3fn():
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(ref.decode_table(), want, equal_nan=True)


@pytest.mark.parametrize("amax", [2.0 ** -24, 2.0 ** -14, 0.5, 1.0, 2.0, 224.0, 256.0, 448.0, 1024.0, 65504.0])
def test_exponent_at_powers_and_448_boundaries(amax):
    h = np.float16(amax)
    for a in {h, np.nextafter(h, np.float16(0))} | ({np.nextafter(h, np.float16(np.inf))} if h < 65504 else set()):
        a = float(a)
        if a == 0:
            continue
        k = int(ref.row_exponent(a))
        assert a <= 448.0 * 2.0 ** k and a > 448.0 * 2.0 ** (k - 1), (a, k)


@pytest.mark.parametrize("j", range(-20, 7))
def test_exponent_around_448_times_power(j):
    b = np.float16(448.0 * 2.0 ** j)
    for a in (b, np.nextafter(b, np.float16(np.inf)), np.nextafter(b, np.float16(0))):
        k = int(ref.row_exponent(float(a)))
        assert float(a) <= 448.0 * 2.0 ** k and float(a) > 448.0 * 2.0 ** (k - 1)


def test_quantize_matches_torch_cast():
    gen = np.random.default_rng(0)
    x = (gen.standard_normal((64, 128)) * np.exp2(gen.integers(-20, 12, (64, 1)))).astype(np.float16)
    x[3] = 65504.0
    x[4, :5] = -65504.0
    x[5] = np.float16(2.0 ** -24) * gen.integers(-3, 4, 128)  # fp16 subnormals
    codes, s = ref.quantize(x)
    live = s > 0
    assert np.array_equal(codes[live], _torch_codes(x[live].astype(np.float64), s[live]))
    assert np.all(np.log2(s[live]) == np.round(np.log2(s[live])))
    back = ref.dequantize(codes, s)
    assert np.all(np.abs(back) <= 448.0 * s[:, None] + 0)
    rel = np.abs(back - x) / np.maximum(np.abs(x).max(-1, keepdims=True), 1e-30)
    assert rel.max() <= 2.0 ** -4  # 3 mantissa bits, relative to the row's max
    assert ref.dequantize_fp16(codes[3:4], s[3:4]).max() == 65504.0  # 65504 rounds up to 256 * 2^8: saturated


def test_zero_nan_inf_rows():
    x = np.zeros((4, 128), np.float16)
    x[1, 7] = np.nan
    x[2, 0] = np.inf
    x[3, 9] = -np.inf
    x[0, 3] = -0.0
    codes, s = ref.quantize(x)
    assert s[0] == 0 and np.all(codes[0] == 0)
    assert np.all(np.isnan(s[1:])) and np.all(codes[1:] == 0)
    assert np.all(np.isnan(ref.dequantize(codes[1:], s[1:])))


def _varied_rows(n=4096, seed=7):
    """rows spanning the fp16 range (scales 2^-24 .. 2^15 times N(0, 1), subnormals, saturating rows), zero rows, NaN / inf rows"""
    gen = np.random.default_rng(seed)
    x = gen.standard_normal((n, 128)) * np.exp2(gen.integers(-30, 16, (n, 1)))
    x = np.clip(x, -65504.0, 65504.0).astype(np.float16)
    x[::97] = 0
    x[5::101, 3] = np.nan
    x[7::103, 11] = np.inf
    x[9::107, 0] = -np.inf
    x[11::109] = np.float16(65504.0) * np.sign(gen.standard_normal(128)).astype(np.float16)
    x[13::113, 1] = -0.0
    return x


def test_torch_form_matches_the_restatement_on_many_rows():
    from autoawq_amd.modules.fused.cache import dequantize_rows_fp8, quantize_rows_fp8

    x = _varied_rows()
    c, s = quantize_rows_fp8(torch.from_numpy(x))
    rc, rs = ref.quantize(x)
    assert np.array_equal(c.numpy(), rc) and np.array_equal(s.numpy(), rs, equal_nan=True)
    assert np.array_equal(dequantize_rows_fp8(c, s).numpy(), ref.dequantize_fp16(rc, rs), equal_nan=True)


def test_torch_form_of_the_cache_matches_the_restatement():
    from autoawq_amd.modules.fused.cache import dequantize_rows_fp8, quantize_rows_fp8

    gen = torch.Generator().manual_seed(1)
    x = (torch.randn((6, 128), generator=gen) * 37).half()
    x[1] = 0
    x[2, 4] = float("nan")
    c, s = quantize_rows_fp8(x)
    rc, rs = ref.quantize(x.numpy())
    assert np.array_equal(c.numpy(), rc) and np.array_equal(s.numpy(), rs, equal_nan=True)
    assert np.array_equal(dequantize_rows_fp8(c, s).numpy(), ref.dequantize_fp16(rc, rs), equal_nan=True)


def _filled_cache(batch=3, T=16, H=2):
    from autoawq_amd.modules.fused.cache import WindowedCache

    c = WindowedCache(batch, H, H, 128, T, "cpu", dtype="fp8")
    gen = torch.Generator().manual_seed(2)
    c.kv.copy_(torch.randint(0, 126, c.kv.shape, generator=gen, dtype=torch.uint8))
    c.scales.copy_(torch.arange(c.scales.numel(), dtype=torch.float32).view(c.scales.shape))  # a scale names its row
    return c


def test_cache_views_and_bytes():
    from autoawq_amd.modules.fused.cache import WindowedCache

    c = WindowedCache(2, 4, 4, 128, 8, "cpu", dtype="fp8")
    f = WindowedCache(2, 4, 4, 128, 8, "cpu")
    assert c.k.dtype == torch.uint8 and c.k_scale.shape == (2, 8, 4) and c.k.data_ptr() == c.kv.data_ptr()
    assert c.v_scale.data_ptr() == c.scales[1].data_ptr()
    assert f.k_scale is None and f.scales is None and f.k.dtype == torch.float16
    nbytes = c.kv.numel() + c.scales.numel() * 4
    assert nbytes / (f.kv.numel() * 2) == pytest.approx(132 / 256)
    with pytest.raises(ValueError):
        WindowedCache(2, 4, 4, 128, 8, "cpu", dtype="fp4")


def test_roll_kv_n_steps_moves_scales_with_rows():
    c = _filled_cache()
    kv0, s0 = c.kv.clone(), c.scales.clone()
    live = c.roll_kv_n_steps(12, n=5)
    assert live == 7
    assert torch.equal(c.kv[:, :, :7], kv0[:, :, 5:12]) and torch.equal(c.scales[:, :, :7], s0[:, :, 5:12])


def test_roll_rows_moves_scales_with_rows():
    c = _filled_cache()
    kv0, s0 = c.kv.clone(), c.scales.clone()
    c.roll_rows([1], 4)
    assert torch.equal(c.kv[:, 1, :12], kv0[:, 1, 4:]) and torch.equal(c.scales[:, 1, :12], s0[:, 1, 4:])
    for r in (0, 2):
        assert torch.equal(c.kv[:, r], kv0[:, r]) and torch.equal(c.scales[:, r], s0[:, r])


def test_batch_resizes_keep_codes_and_scales():
    c = _filled_cache()
    kv0, s0 = c.kv.clone(), c.scales.clone()
    c.decrease_batch_size(2)
    assert torch.equal(c.kv, kv0[:, :2]) and torch.equal(c.scales, s0[:, :2])
    c.increase_batch_size(4)
    assert torch.equal(c.kv[:, :2], kv0[:, :2]) and torch.equal(c.scales[:, :2], s0[:, :2])
    assert not c.scales[:, 2:].any() and c.k_scale.data_ptr() == c.scales.data_ptr()
    c.to("cpu")
    assert torch.equal(c.scales[:, :2], s0[:, :2])


def test_update_get_round_trip():
    c = _filled_cache(batch=2, T=16)
    gen = torch.Generator().manual_seed(3)
    k = (torch.randn((2, 5, 2, 128), generator=gen) * 3).half()
    v = (torch.randn((2, 5, 2, 128), generator=gen) / 7).half()
    c.update_kv(v, k, 2, 4, 5)
    vv, kk = c.get_kv(2, 4, 5)
    assert kk.dtype == torch.float16 and kk.shape == (2, 9, 2, 128)
    assert np.array_equal(kk[:, 4:].numpy(), ref.fake_quant(k.numpy()))
    assert np.array_equal(vv[:, 4:].numpy(), ref.fake_quant(v.numpy()))


def test_attention_rejects_fp8_for_non_native_heads():
    from autoawq_amd.modules.fused.attn import QuantAttentionFused

    def make(n_heads, n_kv, head_dim, dt):
        return QuantAttentionFused(n_heads * head_dim, n_heads, n_kv, None, None, "cpu", max_seq_len=8, head_dim=head_dim,
                                   kv_cache_dtype=dt)

    with pytest.raises(ValueError, match="head_dim 128"):
        make(4, 4, 64, "fp8")
    with pytest.raises(ValueError, match="head_dim 128"):
        make(6, 2, 128, "fp8")  # 3 query heads per KV head
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        make(4, 4, 128, "int8")
    a = make(8, 2, 128, "fp8")
    assert a.kv_cache_dtype == "fp8" and a.cache.k.dtype == torch.uint8
    assert make(6, 2, 128, "fp16").cache.k.dtype == torch.float16


def test_fusers_reject_unknown_dtype():
    from autoawq_amd.fuser import fuse_llama, fuse_mixtral

    for f in (fuse_llama, fuse_mixtral):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            f(None, kv_cache_dtype="e5m2")


def test_ops_reject_mismatched_cache_and_scales():
    from autoawq_amd import ops
    from autoawq_amd._lib import AwqHipError

    c8 = torch.zeros((1, 8, 2, 128), dtype=torch.uint8)
    c16 = torch.zeros((1, 8, 2, 128), dtype=torch.float16)
    s = torch.zeros((1, 8, 2), dtype=torch.float32)
    q = torch.zeros((1, 2, 128), dtype=torch.float16)
    with pytest.raises(AwqHipError, match="k_scale"):
        ops.decode_attention(q, c8, c8, 4)
    with pytest.raises(AwqHipError, match="fp8"):
        ops.decode_attention(q, c16, c16, 4, k_scale=s, v_scale=s)
    with pytest.raises(AwqHipError, match="k_scale"):
        ops.decode_attention_rope(q, c8, c8, None, None, 3, 2, 2, k_scale=s)
    with pytest.raises(AwqHipError, match="scales must be"):
        ops.rope_kv_append(q, c8, c8, None, None, 0, 2, 2, 128, 128, k_scale=s[:, :4], v_scale=s)


NEW_SYMBOLS = ["awq_rope_kv_append_fp8", "awq_rope_kv_append_rows_fp8", "awq_decode_attention_fp8", "awq_decode_attention_ex_fp8",
               "awq_decode_attention_rope_fp8", "awq_decode_attention_rows_fp8", "awq_decode_attention_rope_rows_fp8",
               "awq_kv_quant_fp8", "awq_kv_dequant_fp8"]


def test_new_symbols_in_library_and_table():
    from autoawq_amd import _lib

    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
    so = ctypes.CDLL(os.path.join(os.path.dirname(_lib.__file__), "csrc", "libawq_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(so, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(_lib.__file__)), "include", "awq_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header, name
