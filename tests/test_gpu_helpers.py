"""The helper kernels of csrc/rebin.hip - pu_rebin_time, pu_rebin_chan, pu_roll_rows,
pu_roll_and_sum, pu_transpose - through the C ABI, and their Python wrappers.

Inputs are views into a larger buffer (leading dimension n + 5 and n, base offset 0 and 1
element; the bytes around the view are noise, so a kernel that steps with the wrong stride
reads wrong values).  Outputs lie between two guard regions filled with a byte pattern; the
guards, and the padding of every output row, must be unchanged after the call, which shows an
out-of-bounds write without provoking a fault.  References are explicit numpy loops in the
output dtype and the reference's add order; every comparison is exact."""
import ctypes

import numpy as np
import pytest

from oracle import clean_oracle as co
from pulsarutils import _hip, dedispersion, sigproc

pytestmark = pytest.mark.gpu

PU_OK, PU_EINVAL, PU_EUNSUPPORTED = 0, -1, -4
GUARD, PATTERN = 256, 0xA5
CODES = {"u8": _hip.PU_U8, "f32": _hip.PU_F32, "f64": _hip.PU_F64, "i64": _hip.PU_I64}
NP = {"u8": np.uint8, "f32": np.float32, "f64": np.float64, "i64": np.int64}
VIEWS = [(5, 0), (0, 0), (5, 1), (0, 1)]   # (ld - n, base offset in elements)


def values(rng, dt, shape, w=1):
    """Test values: u8 all 255 (the largest sums), floats with a wide exponent range (every
    add rounds), i64 of both signs above 2**53 / w (so the float64 cast of each element rounds)
    that stay below 2**62 / w (integer sums of w of them do not wrap)."""
    if dt == "u8":
        return np.full(shape, 255, np.uint8)
    if dt == "i64":
        lo, hi = (1 << 54) // w, (1 << 61) // w
        v = rng.integers(lo, hi, size=shape, dtype=np.int64) | 1
        return np.where(rng.random(shape) < 0.5, -v, v)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(NP[dt])


class In:
    """``x`` (nrows, n) laid out with leading dimension ``ld`` at element ``off`` of a device
    buffer whose other elements are noise."""

    def __init__(self, gpu, x, ld, off):
        import torch
        nrows, n = x.shape
        rng = np.random.default_rng(5)
        big = rng.integers(0, 256, size=(off + nrows * ld + 8) * x.itemsize, dtype=np.uint8).view(x.dtype).copy()
        for r in range(nrows):
            big[off + r * ld: off + r * ld + n] = x[r]
        self.buf = torch.from_numpy(big.view(np.uint8)).to(gpu)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + off * x.itemsize)
        self.ld = ld


class Out:
    """``nbytes`` of output between two guards, all filled with the pattern."""

    def __init__(self, gpu, nbytes, init=None):
        import torch
        host = np.full(2 * GUARD + nbytes, PATTERN, np.uint8)
        if init is not None:
            host[GUARD:GUARD + nbytes] = np.ascontiguousarray(init).view(np.uint8).ravel()
        self.nbytes = nbytes
        self.buf = torch.from_numpy(host).to(gpu)
        assert self.buf.data_ptr() % 8 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def read(self, dtype):
        """The payload as ``dtype``, after checking both guards."""
        import torch
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == PATTERN).all(), "write before the output"
        assert (host[GUARD + self.nbytes:] == PATTERN).all(), "write past the output"
        return host[GUARD:GUARD + self.nbytes].view(dtype)

    def untouched(self):
        return (self.read(np.uint8) == PATTERN).all()


def stream():
    return _hip.stream_ptr()


# ------------------------------------------------------------------ pu_rebin_time

def ref_rebin_time(x, w):
    nout = x.shape[1] // w
    out = np.zeros((x.shape[0], nout), np.float64)
    for j in range(w):          # acc = 0.0; acc += (double)p[j], j ascending
        out += x[:, j:nout * w:w].astype(np.float64)
    return out


@pytest.mark.parametrize("dt", ["u8", "f32", "f64", "i64"])
def test_rebin_time(gpu, dt):
    lib = _hip.lib()
    rng = np.random.default_rng(11)
    for nrows in (1, 3):
        for n in (1, 255, 256, 257, 1003):
            for w in sorted({1, 2, 3, 7, 8, n, n + 1}):
                x = values(rng, dt, (nrows, n), w)
                want = ref_rebin_time(x, w)
                for pad, off in VIEWS:
                    src = In(gpu, x, n + pad, off)
                    out = Out(gpu, max(want.size, 1) * 8)
                    rc = lib.pu_rebin_time(src.ptr, CODES[dt], nrows, n, src.ld, w, out.ptr, stream())
                    assert rc == PU_OK, (nrows, n, w, pad, off)
                    if want.size == 0:      # w > n: no output, nothing written
                        assert w > n and out.untouched()
                        continue
                    got = out.read(np.float64).reshape(want.shape)
                    assert np.array_equal(got, want), (nrows, n, w, pad, off, np.argwhere(got != want)[:5].tolist())
    if dt == "i64":   # the values are such that the per-element cast differs from a cast of the integer sum
        x = values(rng, dt, (3, 1003), 7)
        exact = x[:, :1001].reshape(3, 143, 7).sum(2).astype(np.float64)
        assert (exact != ref_rebin_time(x, 7)).any()


# ------------------------------------------------------------------ pu_rebin_chan

OUT_CHAN = {"u8": np.uint64, "f32": np.float32, "f64": np.float64, "i64": np.int64}


def ref_rebin_chan(x, rb, out_dtype):
    ng = x.shape[0] // rb
    out = x[0:ng * rb:rb].astype(out_dtype)      # acc = (Tout)p[0]
    for j in range(1, rb):                       # acc += (Tout)p[j * ld], j ascending
        out = out + x[j:ng * rb:rb].astype(out_dtype)
    assert out.dtype == out_dtype
    return out


@pytest.mark.parametrize("dt", ["u8", "f32", "f64", "i64"])
def test_rebin_chan(gpu, dt):
    lib = _hip.lib()
    rng = np.random.default_rng(12)
    nrows = 7
    for n in (1, 257, 1003):
        for rb in (1, 2, 3, 7, 8):
            x = values(rng, dt, (nrows, n), rb)
            want = ref_rebin_chan(x, rb, OUT_CHAN[dt])
            for pad, off in VIEWS:
                src = In(gpu, x, n + pad, off)
                out = Out(gpu, max(want.size, 1) * 8)
                rc = lib.pu_rebin_chan(src.ptr, CODES[dt], nrows, n, src.ld, rb, out.ptr, stream())
                assert rc == PU_OK, (n, rb, pad, off)
                if want.size == 0:          # rb > nrows: no output group
                    assert rb == 8 and out.untouched()
                    continue
                got = out.read(np.uint8)[:want.nbytes].view(OUT_CHAN[dt]).reshape(want.shape)
                assert np.array_equal(got, want), (n, rb, pad, off, np.argwhere(got != want)[:5].tolist())
                assert (out.read(np.uint8)[want.nbytes:] == PATTERN).all()
    if dt == "u8":
        assert ref_rebin_chan(values(rng, dt, (7, 4)), 7, np.uint64).max() == 7 * 255   # above 255: not a uint8 sum
    if dt == "i64":
        assert (values(rng, dt, (7, 100)) < 0).any()
    if dt == "f32":   # sequential float32 adds differ from a float64 sum rounded once
        x = values(rng, dt, (7, 1003))
        assert (ref_rebin_chan(x, 7, np.float32) != x.astype(np.float64).sum(0).astype(np.float32)).any()


# ------------------------------------------------------------------ pu_roll_rows

def roll_payload(rng, dt, nrows, n):
    """Random bits with NaN, -0.0 and inf patterns among them (compared as bytes)."""
    x = rng.integers(0, 256, size=nrows * n * np.dtype(NP[dt]).itemsize, dtype=np.uint8).view(NP[dt]).reshape(nrows, n)
    x = x.copy()
    if dt in ("f32", "f64"):
        flat = x.reshape(-1)
        for k, v in enumerate((np.nan, -0.0, np.inf, -np.nan)):
            flat[(k * 7) % flat.size] = v
    return x


@pytest.mark.parametrize("dt", ["u8", "f32", "f64", "i64"])
def test_roll_rows(gpu, dt):
    """out[r, t] = x[r, (t + shift[r]) mod n] (np.roll by -shift) on 1-, 4- and 8-byte elements."""
    import torch
    lib = _hip.lib()
    rng = np.random.default_rng(13)
    for n in (1, 2, 256, 1003):
        big = (1 << 40) + 3
        shifts = [0, 1, -1, n - 1, -(n - 1), n, -n, n + 1, -(n + 1), big, -big]
        shifts = np.array(shifts[3:] + shifts[:3], dtype=np.int64)   # mixed per row
        nrows = shifts.size
        x = roll_payload(rng, dt, nrows, n)
        want = np.stack([x[r, (np.arange(n) + int(shifts[r])) % n] for r in range(nrows)])
        for r in range(nrows):
            assert want[r].tobytes() == np.roll(x[r], -int(shifts[r])).tobytes()
        dsh = torch.from_numpy(shifts).to(gpu)
        for pad, off in VIEWS:
            src = In(gpu, x, n + pad, off)
            out = Out(gpu, want.nbytes)
            rc = lib.pu_roll_rows(src.ptr, CODES[dt], nrows, n, src.ld, _hip.ptr(dsh), out.ptr, stream())
            assert rc == PU_OK, (n, pad, off)
            got = out.read(np.uint8)
            assert got.tobytes() == want.tobytes(), (n, pad, off)


# ------------------------------------------------------------------ pu_roll_and_sum

@pytest.mark.parametrize("dt", ["u8", "f32", "f64", "i64"])
def test_roll_and_sum(gpu, dt):
    """sum[t] += (double)x[(t - roll) mod n] on a non-zero sum; a roll outside [0, n) is refused
    and leaves the sum as it was."""
    lib = _hip.lib()
    rng = np.random.default_rng(14)
    for n in (1, 2, 257, 1003):
        x = values(rng, dt, (1, n))
        if dt == "u8":
            x = rng.integers(0, 256, size=(1, n), dtype=np.uint8)
        sum0 = rng.standard_normal(n) * 1000.0
        for off in (0, 1):
            src = In(gpu, x, n, off)
            for roll in sorted({0, 1, n - 1} & set(range(n))):
                want = sum0 + np.roll(x[0], roll).astype(np.float64)
                out = Out(gpu, n * 8, init=sum0)
                rc = lib.pu_roll_and_sum(src.ptr, CODES[dt], n, roll, out.ptr, stream())
                assert rc == PU_OK, (n, roll, off)
                got = out.read(np.float64)
                assert np.array_equal(got, want), (n, roll, off)
                assert roll == 0 or n < 3 or not np.array_equal(got, sum0 + x[0].astype(np.float64))
            for roll in (n, -1):
                out = Out(gpu, n * 8, init=sum0)
                assert lib.pu_roll_and_sum(src.ptr, CODES[dt], n, roll, out.ptr, stream()) == PU_EINVAL
                assert np.array_equal(out.read(np.float64), sum0)


# ------------------------------------------------------------------ pu_transpose

SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (65, 130), (777, 130)]


@pytest.mark.parametrize("esize", [1, 2, 4, 8])
def test_transpose(gpu, esize):
    lib = _hip.lib()
    rng = np.random.default_rng(15)
    dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[esize]
    for rows, cols in SHAPES:
        x = rng.integers(0, 256, size=rows * cols * esize, dtype=np.uint8).view(dtype).reshape(rows, cols)
        for (pad, off), pad_dst in zip(VIEWS, (3, 0, 0, 3)):
            src = In(gpu, x, cols + pad, off)
            ld_dst = rows + pad_dst
            out = Out(gpu, cols * ld_dst * esize)
            rc = lib.pu_transpose(src.ptr, esize, rows, cols, src.ld, out.ptr, ld_dst, stream())
            assert rc == PU_OK, (rows, cols, pad, off)
            got = out.read(dtype).reshape(cols, ld_dst)
            assert np.array_equal(got[:, :rows], x.T), (rows, cols, pad, off, pad_dst)
            assert (np.ascontiguousarray(got[:, rows:]).view(np.uint8) == PATTERN).all(), "dst row padding written"


def test_transpose_unsupported_element_size(gpu):
    x = np.arange(30, dtype=np.uint8).reshape(2, 15)
    src = In(gpu, x, 15, 0)
    out = Out(gpu, 30)
    assert _hip.lib().pu_transpose(src.ptr, 3, 2, 5, 5, out.ptr, 2, stream()) == PU_EUNSUPPORTED
    assert out.untouched()


# ------------------------------------------------------------------ the Python wrappers

def wrapper_inputs(gpu):
    """(name, numpy array, the same as a torch tensor or None): int16, int32, bool, uint16 and
    big-endian float64, 7 x 53, with negative and large values."""
    import torch
    rng = np.random.default_rng(16)
    base = rng.integers(-30000, 30000, size=(7, 53))
    cases = [("int16", base.astype(np.int16)), ("int32", (base * 60000).astype(np.int32)),
             ("bool", base > 0), ("uint16", (base + 30000).astype(np.uint16)),
             (">f8", (base * 1e-3 + 0.1).astype(">f8"))]
    out = []
    for name, a in cases:
        out.append((name + "-numpy", a, a))
        if name != ">f8":   # (torch has no byte-swapped dtypes)
            out.append((name + "-torch-cpu", a, torch.from_numpy(a.copy())))
            out.append((name + "-torch-gpu", a, torch.from_numpy(a.copy()).to(gpu)))
    return out


def test_wrappers_follow_numpy_dtypes(gpu):
    """quick_chan_rebin: np.sum's dtype rules; quick_resample: float64; apply_dm_shifts_to_data:
    the input's dtype - values and dtypes equal numpy's on the same input, for numpy arrays and
    torch tensors (host and device) of the dtypes the kernels do not take directly."""
    shifts = np.array([0.0, 1.4, -1.6, 52.0, 53.0, -107.5, 1e6 + 3])
    for name, a, arg in wrapper_inputs(gpu):
        for rb in (1, 3):
            want = co.quick_chan_rebin(a, rb)
            got = dedispersion.quick_chan_rebin(arg, rb)
            assert isinstance(got, np.ndarray) and got.dtype == want.dtype, (name, rb, got.dtype, want.dtype)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} chan {rb}")
        for w in (1, 4):
            want = co.quick_resample(a, w)
            got = dedispersion.quick_resample(arg, w)
            assert got.dtype == np.float64 and want.dtype == np.float64, (name, w)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} time {w}")
        want = co.apply_dm_shifts(a, shifts)
        got = dedispersion.apply_dm_shifts_to_data(arg, shifts)
        assert got.dtype == a.dtype == want.dtype, (name, got.dtype, a.dtype)
        assert got.tobytes() == want.tobytes(), name


def test_roll_and_sum_wrapper_edges(gpu):
    """roll_and_sum with N = 0 and N = size (np.roll by the whole length: no roll), and in between."""
    rng = np.random.default_rng(17)
    for a in (rng.integers(-30000, 30000, size=301).astype(np.int16), rng.standard_normal(301).astype(">f8"),
              rng.random(301) > 0.5, rng.integers(0, 60000, size=301).astype(np.uint16)):
        for N in (0, 301, 1, 300):
            s0 = rng.standard_normal(301)
            s = s0.copy()
            res = dedispersion.roll_and_sum(a, s, N)
            assert res is s
            np.testing.assert_array_equal(s, s0 + np.roll(a, N), err_msg=f"{a.dtype} N={N}")
    for N in (-1, 302):
        with pytest.raises(IndexError):
            dedispersion.roll_and_sum(np.zeros(301), np.zeros(301), N)


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32, np.float64])
def test_transpose_device_views(gpu, dt):
    """transpose_device on views: a row-strided one, single rows (whose row stride torch leaves
    arbitrary), and a column-strided one, which is transposed correctly or refused - never
    transposed as if its columns were adjacent."""
    import torch
    rng = np.random.default_rng(18)
    x = (rng.random((130, 77)) * 250).astype(dt)
    xd = torch.from_numpy(x).to(gpu)
    view = xd[:, 3:70]
    assert view.stride() == (77, 1)
    np.testing.assert_array_equal(sigproc.transpose_device(view).cpu().numpy(), x[:, 3:70].T)
    np.testing.assert_array_equal(sigproc.transpose_device(xd[5:6, 3:70]).cpu().numpy(), x[5:6, 3:70].T)
    row = xd[:, 4:5].t()            # (1, 130) with strides (1, 77): a single row
    assert row.shape == (1, 130)
    try:
        got = sigproc.transpose_device(row)
    except ValueError:
        pass
    else:
        np.testing.assert_array_equal(got.cpu().numpy(), x[:, 4:5])
    row = xd[7].reshape(77, 1).t()  # (1, 77), unit column stride, row stride 1 < 77
    assert row.shape == (1, 77) and row.stride(1) == 1
    np.testing.assert_array_equal(sigproc.transpose_device(row).cpu().numpy(), x[7].reshape(77, 1))
    cols = xd[:, ::2]
    assert cols.stride() == (77, 2)
    try:
        got = sigproc.transpose_device(cols)
    except ValueError:
        pass
    else:
        np.testing.assert_array_equal(got.cpu().numpy(), x[:, ::2].T)
