"""pu_quantize_pack_transpose (quantise + transpose + pack of a channel-major block, the
inverse of pu_unpack_transpose) against a numpy restatement of the formula in
include/pulsarutils_hip.h.  Every comparison is exact."""
import numpy as np
import pytest

from pulsarutils import sigproc

pytestmark = pytest.mark.gpu

# (nsamps, nchans): a single spectrum (one byte per row at 1 bit); just past 64 samples; 3-byte
# rows at 1 bit; ragged against the 128-sample x 128-channel tile both ways; wide rows (several
# channel tiles); a prime sample count over 33 time tiles
SHAPES = [(1, 8), (65, 8), (300, 24), (777, 136), (64, 4096), (4099, 64)]
# 5-byte rows: the stores cannot be wider than a byte.  (400, 256): whole tiles behind 16-byte
# aligned rows, so every dtype takes its widest loads (none of SHAPES has both)
CASES = ([(nbits,) + s for nbits in (1, 2, 4, 8) for s in SHAPES] + [(2, 300, 20), (1, 300, 40)]
         + [(nbits, 400, 256) for nbits in (1, 2, 4, 8)])
DTYPES = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}


def levels(nbits, nchans, seed):
    """Power-of-two scales and half-integer offsets of either sign: with inputs that are
    multiples of 0.25, v = x * scale + offset is exact in float64 and often an exact .5 tie."""
    rng = np.random.default_rng(seed)
    scale = np.ldexp(1.0, rng.integers(-1, 2, size=nchans))          # 0.5, 1, 2
    offset = rng.integers(-(1 << nbits), 1 << nbits, size=nchans) + 0.5
    return scale, offset


def plane(dt, nbits, nchans, nsamps, seed):
    """(nchans, nsamps) input: multiples of 0.25 spread well past both clip levels (uint8:
    integers, some far above the top level of every width)."""
    rng = np.random.default_rng(seed)
    top = (1 << nbits) - 1
    if dt == np.uint8:
        return rng.integers(0, min(255, 3 * top + 4) + 1, size=(nchans, nsamps)).astype(np.uint8)
    return (rng.integers(-8 * (top + 4), 8 * (top + 4) + 1, size=(nchans, nsamps)) * 0.25).astype(dt)


def quantised(x, nbits, scale=None, offset=None):
    """The header's formula: (q (nchans, nsamps) uint8, v)."""
    top = (1 << nbits) - 1
    if scale is None:
        v = x.astype(np.float64)
        v_fixed = np.where(np.isnan(v), 0.0, v)
    else:
        with np.errstate(invalid="ignore"):       # (inf * 0 is one of the special values)
            v = x.astype(np.float64) * scale[:, None] + offset[:, None]
        v_fixed = np.where(np.isnan(v), offset[:, None], v)
    return np.clip(np.rint(v_fixed), 0, top).astype(np.uint8), v


def packed_rows(q, nbits):
    return np.ascontiguousarray(q.T) if nbits == 8 else sigproc._pack(q.T, nbits)


def run(x, nbits, scale, offset, gpu):
    import torch
    return sigproc.quantize_pack_device(torch.from_numpy(x).to(gpu), nbits, scale, offset).cpu().numpy()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nbits,nsamps,nchans", CASES)
def test_quantize_shapes(gpu, nbits, nsamps, nchans, dt):
    import torch
    top = (1 << nbits) - 1
    x = plane(DTYPES[dt], nbits, nchans, nsamps, seed=nbits * 11 + nsamps)
    scale, offset = levels(nbits, nchans, seed=100 + nchans + nbits)
    q, v = quantised(x, nbits, scale, offset)
    if nsamps * nchans >= 512:
        # the case exercises what it is meant to: both clip levels, and ties that half-to-even
        # and half-away-from-zero round differently (an even integer + 0.5 inside the range)
        frac_half = (v - np.floor(v) == 0.5) & (v > 0) & (v < top) & (np.floor(v) % 2 == 0)
        assert (q == 0).any() and (q == top).any() and (v < -0.5).any() and (v > top + 0.5).any()
        assert frac_half.any()
    out = sigproc.quantize_pack_device(torch.from_numpy(x).to(gpu), nbits, scale, offset)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (nsamps, nchans * nbits // 8) and out.is_contiguous()
    np.testing.assert_array_equal(out.cpu().numpy(), packed_rows(q, nbits))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("identity", [False, True])
def test_float32_output(gpu, dt, identity):
    import torch
    nsamps, nchans = 777, 136
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((nchans, nsamps)) * 1e3).astype(DTYPES[dt])
    x[3, 5], x[100, 700], x[135, 776] = np.nan, np.inf, -np.inf
    scale = rng.uniform(0.1, 3.0, nchans)
    offset = rng.uniform(-5.0, 5.0, nchans)
    if identity:
        want = x.astype(np.float64).astype(np.float32).T
        out = sigproc.quantize_pack_device(torch.from_numpy(x).to(gpu), 32)
    else:
        want = (x.astype(np.float64) * scale[:, None] + offset[:, None]).astype(np.float32).T
        out = sigproc.quantize_pack_device(torch.from_numpy(x).to(gpu), 32, scale, offset)
    assert out.dtype == torch.float32 and tuple(out.shape) == (nsamps, nchans) and out.is_contiguous()
    got = out.cpu().numpy()
    assert np.isnan(got[5, 3]) and np.isnan(want[5, 3])
    np.testing.assert_array_equal(got, want)  # (NaNs at equal positions compare equal)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_special_values(gpu, dt, nbits):
    """NaN -> rint(offset[c]) clipped (0 in identity mode), +inf -> top, -inf -> 0; scale 0
    times inf is a NaN too."""
    nsamps, nchans = 300, 24
    top = (1 << nbits) - 1
    x = plane(DTYPES[dt], nbits, nchans, nsamps, seed=17 + nbits)
    scale, offset = levels(nbits, nchans, seed=3)
    offset[7] = top + 10.5                  # a NaN of channel 7 clips to top
    scale[9] = 0.0
    spots = {(2, 0): np.nan, (7, 11): np.nan, (5, 299): np.inf, (6, 150): -np.inf, (9, 33): np.inf}
    for (c, t_), val in spots.items():
        x[c, t_] = val
    q, _ = quantised(x, nbits, scale, offset)
    assert q[2, 0] == np.clip(np.rint(offset[2]), 0, top) and q[7, 11] == top and q[5, 299] == top
    assert q[6, 150] == 0 and q[9, 33] == np.clip(np.rint(offset[9]), 0, top)
    np.testing.assert_array_equal(run(x, nbits, scale, offset, gpu), packed_rows(q, nbits))
    qi, _ = quantised(x, nbits)
    assert qi[2, 0] == 0 and qi[5, 299] == top and qi[6, 150] == 0
    np.testing.assert_array_equal(run(x, nbits, None, None, gpu), packed_rows(qi, nbits))


def _raw_call(src, nchans, nsamps, ld_src, scale, offset, nbits, dst, ld_dst, stream=None):
    from pulsarutils import _hip
    _hip.check(_hip.lib().pu_quantize_pack_transpose(_hip.ptr(src), _hip.dtype_code(src.dtype), nchans, nsamps, ld_src,
                                                     _hip.ptr(scale), _hip.ptr(offset), nbits, _hip.ptr(dst), ld_dst,
                                                     _hip.stream_ptr(stream)), "pu_quantize_pack_transpose")


def _case(gpu, nbits, nsamps=777, nchans=136, dt=np.float64, seed=0):
    import torch
    x = plane(dt, nbits, nchans, nsamps, seed=seed + nbits)
    scale, offset = levels(nbits, nchans, seed=seed + 1)
    q, _ = quantised(x, nbits, scale, offset)
    return x, torch.from_numpy(scale).to(gpu), torch.from_numpy(offset).to(gpu), packed_rows(q, nbits)


@pytest.mark.parametrize("nbits", [1, 2, 4, 8, 32])
def test_padded_ld_dst_untouched(gpu, nbits):
    import torch
    nsamps, nchans = 777, 136
    x, ds, do, want = _case(gpu, min(nbits, 8), seed=40)
    rb = nchans * nbits // 8
    pad = 12 if nbits == 32 else 13
    dst = torch.full((nsamps, rb + pad), 0xAB, dtype=torch.uint8, device=gpu)
    _raw_call(torch.from_numpy(x).to(gpu), nchans, nsamps, nsamps, ds, do, nbits, dst, rb + pad)
    got = dst.cpu().numpy()
    if nbits == 32:
        want = (x * ds.cpu().numpy()[:, None] + do.cpu().numpy()[:, None]).astype(np.float32).T
        want = np.ascontiguousarray(want).view(np.uint8)
    np.testing.assert_array_equal(got[:, :rb], want)
    assert np.all(got[:, rb:] == 0xAB)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_padded_ld_src(gpu, nbits, dt):
    """Rows padded by 3 elements (a view of a wider tensor): the row starts lose their
    16-byte alignment and the padding is not read as samples."""
    import torch
    nsamps, nchans = 777, 136
    wide = plane(DTYPES[dt], nbits, nchans, nsamps + 3, seed=50 + nbits)
    scale, offset = levels(nbits, nchans, seed=51)
    view = torch.from_numpy(wide).to(gpu)[:, :nsamps]
    assert view.stride(0) == nsamps + 3
    q, _ = quantised(wide[:, :nsamps], nbits, scale, offset)
    out = sigproc.quantize_pack_device(view, nbits, scale, offset)
    np.testing.assert_array_equal(out.cpu().numpy(), packed_rows(q, nbits))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_src_offset_by_one_element(gpu, nbits, dt):
    import torch
    nsamps, nchans = 384, 128            # whole tiles and 16-byte row pitches: only the pointer is misaligned
    flat = plane(DTYPES[dt], nbits, 1, nchans * nsamps + 1, seed=60 + nbits)[0]
    scale, offset = levels(nbits, nchans, seed=61)
    view = torch.from_numpy(flat).to(gpu)[1:].view(nchans, nsamps)
    assert view.data_ptr() % 16 == flat.itemsize
    q, _ = quantised(flat[1:].reshape(nchans, nsamps), nbits, scale, offset)
    out = sigproc.quantize_pack_device(view, nbits, scale, offset)
    np.testing.assert_array_equal(out.cpu().numpy(), packed_rows(q, nbits))


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_dst_offset_by_one_byte(gpu, nbits):
    import torch
    nsamps, nchans = 384, 128
    x, ds, do, want = _case(gpu, nbits, nsamps, nchans, seed=70)
    rb = nchans * nbits // 8
    flat = torch.full((nsamps * rb + 2,), 0xCD, dtype=torch.uint8, device=gpu)
    dst = flat[1:1 + nsamps * rb].view(nsamps, rb)
    assert dst.data_ptr() % 2 == 1
    _raw_call(torch.from_numpy(x).to(gpu), nchans, nsamps, nsamps, ds, do, nbits, dst, rb)
    got = flat.cpu().numpy()
    np.testing.assert_array_equal(got[1:-1].reshape(nsamps, rb), want)
    assert got[0] == 0xCD and got[-1] == 0xCD


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_non_default_stream(gpu, nbits):
    import torch
    x, ds, do, want = _case(gpu, nbits, seed=80)
    dx = torch.from_numpy(x).to(gpu)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        out = sigproc.quantize_pack_device(dx, nbits, ds, do)
    side.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_empty_block_and_argument_errors(gpu):
    import torch
    out = sigproc.quantize_pack_device(torch.empty((16, 0), dtype=torch.float64, device=gpu), 2)
    assert tuple(out.shape) == (0, 4) and out.dtype == torch.uint8
    out = sigproc.quantize_pack_device(torch.empty((16, 0), dtype=torch.float64, device=gpu), 32)
    assert tuple(out.shape) == (0, 16) and out.dtype == torch.float32
    x = torch.zeros((8, 4), dtype=torch.float64, device=gpu)
    ones = np.ones(8)
    with pytest.raises(ValueError, match="pu_quantize_pack_transpose"):
        sigproc.quantize_pack_device(x, 3)
    with pytest.raises(ValueError, match="whole number of bytes"):
        sigproc.quantize_pack_device(x[:7], 2)
    with pytest.raises(ValueError, match="scale and offset"):
        sigproc.quantize_pack_device(x, 8, scale=ones)
    with pytest.raises(ValueError, match="scale and offset"):
        sigproc.quantize_pack_device(x, 8, offset=ones)
    dst = torch.zeros((4, 8), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="leading dimension"):
        _raw_call(x, 8, 4, 3, None, None, 8, dst, 8)      # ld_src < nsamps
    with pytest.raises(ValueError, match="leading dimension"):
        _raw_call(x, 8, 4, 4, None, None, 8, dst, 7)      # ld_dst < row bytes
    with pytest.raises(ValueError):
        sigproc.quantize_pack_device(x.to(torch.int64), 8)


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_round_trip_through_unpack(gpu, nbits):
    import torch
    nsamps, nchans = 777, 136
    x = plane(np.float64, nbits, nchans, nsamps, seed=90 + nbits)
    scale, offset = levels(nbits, nchans, seed=91)
    q, _ = quantised(x, nbits, scale, offset)
    packed = sigproc.quantize_pack_device(torch.from_numpy(x).to(gpu), nbits, scale, offset)
    back = sigproc.unpack_transpose_device(packed, nbits, nchans)
    np.testing.assert_array_equal(back.cpu().numpy(), q)
