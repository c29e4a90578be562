"""pu_resample_accel, pu_rfft_accel and the acceleration search of pulsarutils.periodicity on the GPU.

The gather is compared bit for bit with tests/accel_oracle.py; the fused transform bit for bit with
pu_rfft of the gathered series (whose accuracy tests/test_gpu_spectrum.py holds to its bound); the
search end to end on the scenario tests/test_accel_oracle.py proves sound on the host."""
import numpy as np
import pytest

import accel_oracle as ao

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu):
    from pulsarutils import _hip
    _hip.require_gpu()
    return _hip


def _device_rows(x, ld):
    """(rows, n) numpy -> a device view with leading dimension ``ld``, the gap filled with NaN."""
    import torch
    rows, n = x.shape
    buf = torch.full((rows, ld), float("nan"), dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    buf[:, :n] = torch.from_numpy(x).cuda()
    return buf[:, :n]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gpu_resample(hip, x, afac, ld=None, ld_out=None):
    """pu_resample_accel through the C ABI: (the (nacc * rows, n) rows, the gaps of the output)."""
    import torch
    rows, n = x.shape
    xd = _device_rows(x, n + 5 if ld is None else ld)
    ld_out = n + 3 if ld_out is None else ld_out
    af = torch.from_numpy(np.asarray(afac, dtype=np.float64)).cuda()
    out = torch.full((af.numel() * rows, ld_out), float("nan"), dtype=xd.dtype, device="cuda")
    hip.check(hip.lib().pu_resample_accel(hip.ptr(xd), hip.dtype_code(xd.dtype), rows, n, xd.stride(0), hip.ptr(af),
                                          af.numel(), hip.ptr(out), ld_out, hip.stream_ptr()), "pu_resample_accel")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return out[:, :n], out[:, n:]


def gpu_rfft(hip, x, nfft, mean, afac=None, ld=None, ld_spec=None):
    """pu_rfft (``afac`` None) or pu_rfft_accel through the C ABI: complex64 numpy (rows or nacc *
    rows, nfft / 2 + 1); input and output rows padded, the gaps NaN."""
    import torch
    from pulsarutils import periodicity as pe
    rows, n = x.shape
    xd = _device_rows(x, n + 7 if ld is None else ld)
    ld_spec = nfft // 2 + 4 if ld_spec is None else ld_spec
    md = torch.from_numpy(np.asarray(mean, dtype=np.float64)).cuda()
    lib = hip.lib()
    if afac is None:
        spec = torch.full((rows, ld_spec), float("nan"), dtype=torch.complex64, device="cuda")
        ws, wp, wsb = hip.workspace(lib.pu_rfft_workspace_bytes(rows, nfft), xd.device)
        hip.check(lib.pu_rfft(hip.ptr(xd), hip.dtype_code(xd.dtype), rows, n, xd.stride(0), hip.ptr(md), nfft,
                              hip.ptr(spec), ld_spec, wp, wsb, hip.stream_ptr()), "pu_rfft")
    else:
        af = torch.from_numpy(np.asarray(afac, dtype=np.float64)).cuda()
        spec = torch.full((af.numel() * rows, ld_spec), float("nan"), dtype=torch.complex64, device="cuda")
        ws, wp, wsb = hip.workspace(lib.pu_rfft_accel_workspace_bytes(rows, af.numel(), nfft), xd.device)
        hip.check(lib.pu_rfft_accel(hip.ptr(xd), hip.dtype_code(xd.dtype), rows, n, xd.stride(0), hip.ptr(md), hip.ptr(af),
                                    af.numel(), nfft, hip.ptr(spec), ld_spec, wp, wsb, hip.stream_ptr()), "pu_rfft_accel")
    torch.cuda.synchronize()
    return spec[:, :nfft // 2 + 1].cpu().numpy()


# ------------------------------------------------------------------ the gather

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [257, 4099])
def test_gather_bit_for_bit(hip, n, dtype):
    """n = 257: two blocks of 256, the second with one sample; 4099: 17 blocks, odd.  2e-3 n > 1:
    the clamp engages; NaN: every sample reads sample 0."""
    afac = [0.0, 3e-5, -3e-5, 2e-3, float("nan")]
    x = np.random.default_rng(n).standard_normal((3, n)).astype(dtype)
    got, gaps = gpu_resample(hip, x, afac)
    assert np.all(np.isnan(gaps))
    want = np.concatenate([ao.resample(x, af) for af in afac])
    assert got.dtype == want.dtype and got.shape == want.shape == (15, n)
    assert got.tobytes() == want.tobytes()      # (no NaN left: nothing read from a gap, no write skipped)
    assert np.array_equal(got[:3], x)           # af = 0 is the identity
    assert np.array_equal(got[12:], np.repeat(x[:, :1], n, axis=1))
    # (the trials are not the identity: 3e-5 n^2 / 4 is half a sample at 257 and 126 samples at 4099)
    moved = [int(np.sum(ao.resample_indices(n, af) != np.arange(n))) for af in afac[1:4]]
    assert moved[2] >= n - 1 and (n == 257 or min(moved) > n // 2), moved


# ------------------------------------------------------------------ the fused transform

def _series(n, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, n)) + np.array([[0.0], [40.0], [-3.0]])
    x[0] += 2.0 * np.cos(2 * np.pi * 0.0712345 * np.arange(n))
    x = x.astype(dtype)
    return x, x.astype(np.float64).sum(axis=1) / n


CASES = [(2 ** 8, 256), (2 ** 8, 233), (2 ** 13, 2 ** 13 - 24), (2 ** 14, 2 ** 14 - 24), (2 ** 14, 2 ** 13 + 1)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nfft, n", CASES)
def test_fused_transform_bit_for_bit_with_two_steps(hip, nfft, n, dtype):
    """2^8 and 2^13: one pass (2^13 its largest); 2^14: the smallest four-step.  n = 233 and
    2^13 + 1 are odd: the last packed pair straddles n.  |af| n = 0.5: a sample moves up to n / 8."""
    x, mean = _series(n, dtype, nfft + n)
    afac = [0.0, 0.5 / n, -0.5 / n]
    fused = gpu_rfft(hip, x, nfft, mean, afac=afac)
    assert fused.shape == (9, nfft // 2 + 1) and np.all(np.isfinite(fused.view(np.float32)))
    gathered, _ = gpu_resample(hip, x, afac)
    assert np.array_equal(gathered, np.concatenate([ao.resample(x, af) for af in afac]))
    two_step = gpu_rfft(hip, np.ascontiguousarray(gathered), nfft, np.tile(mean, 3), ld=n + 2, ld_spec=nfft // 2 + 1)
    assert np.array_equal(_bits(fused), _bits(two_step))
    # the trials differ from one another, and af = 0 is pu_rfft itself
    assert not np.array_equal(_bits(fused[:3]), _bits(fused[3:6]))
    assert not np.array_equal(_bits(fused[3:6]), _bits(fused[6:]))
    plain = gpu_rfft(hip, x, nfft, mean)
    assert np.array_equal(_bits(fused[:3]), _bits(plain))
    # one (acceleration, row) pair alone has the bits it has in the batch
    alone = gpu_rfft(hip, x[1:2], nfft, mean[1:2], afac=afac[2:], ld=n + 64, ld_spec=nfft // 2 + 9)
    assert np.array_equal(_bits(alone), _bits(fused[7:8]))


# ------------------------------------------------------------------ end to end, API

@pytest.fixture(scope="module")
def scenario():
    x = ao.drifting_rows()
    x.setflags(write=False)
    return x


def test_end_to_end_drifting_pulse_train(hip, scenario):
    from pulsarutils import periodicity as pe
    x, dt = scenario, ao.DT
    tobs = ao.N * dt
    grid = pe.acceleration_grid(4e5, tobs, 16 * ao.F0)
    step = grid[1] - grid[0]
    tab = pe.acceleration_search(x, dt, accels=grid, nharm=16, sigma=8)
    print(f"{grid.size} trials, step {step:.1f}; {len(tab)} candidates; best: row {tab['row'][0]} nharm {tab['nharm'][0]} "
          f"freq {tab['freq'][0]:.4f} accel {tab['accel'][0]:.0f} sigma {tab['sigma'][0]:.1f}")
    assert len(tab) >= 1 and np.all(np.diff(tab["logp"]) >= 0)
    assert tab["row"][0] == 0 and tab["nharm"][0] == 16
    assert abs(tab["freq"][0] - ao.F0) <= 1 / (16 * tobs)
    assert abs(tab["accel"][0] - ao.ACCEL) <= step
    assert not np.any(tab["row"] == 1)
    none = pe.periodicity_search(x, dt, nharm=16, sigma=8)
    assert len(none) == 0


def test_api_conventions_and_errors(hip, scenario):
    import torch
    from pulsarutils import periodicity as pe
    x, dt = scenario, ao.DT
    n = x.shape[1]
    xd = torch.from_numpy(x).cuda()
    accels = np.array([-2e5, 0.0, 3.8e5])
    af = ao.accel_factor(accels, dt)
    # resample: a scalar keeps the shape, an array adds an axis in front; numpy in, numpy out
    one = pe.resample(x, 3.8e5, dt)
    assert isinstance(one, np.ndarray) and one.dtype == x.dtype and np.array_equal(one, ao.resample(x, af[2]))
    many = pe.resample(x, accels, dt)
    assert many.shape == (3, 2, n) and all(np.array_equal(many[a], ao.resample(x, af[a])) for a in range(3))
    assert np.array_equal(many[1], x)
    assert pe.resample(x[0], 3.8e5, dt).shape == (n,) and pe.resample(x[0], accels, dt).shape == (3, n)
    x64 = pe.resample(x.astype(np.float64), -2e5, dt)
    assert x64.dtype == np.float64 and np.array_equal(x64, ao.resample(x.astype(np.float64), af[0]))
    md = pe.resample(xd, accels, dt)
    assert isinstance(md, torch.Tensor) and md.is_cuda and np.array_equal(md.cpu().numpy(), many)
    # rfft_accel: the spectrum of each trial, the row's own mean taken out
    spec = pe.rfft_accel(x, accels, dt)
    assert isinstance(spec, np.ndarray) and spec.dtype == np.complex64 and spec.shape == (3, 2, n // 2 + 1)
    assert np.array_equal(_bits(spec[1]), _bits(pe.rfft(x)))
    from pulsarutils.stats import _chunk_row_sums
    mean = (_chunk_row_sums(xd, 3) / float(n)).cpu().numpy()   # the row means as rfft takes them
    want = gpu_rfft(hip, np.ascontiguousarray(many.reshape(6, n)), n, np.tile(mean, 3), ld_spec=n // 2 + 1)
    assert np.array_equal(_bits(spec.reshape(6, -1)), _bits(want))
    assert pe.rfft_accel(x[0], accels, dt, nfft=2 * n).shape == (3, n + 1)
    sd = pe.rfft_accel(xd, accels, dt)
    assert isinstance(sd, torch.Tensor) and sd.is_cuda and np.array_equal(_bits(sd.cpu().numpy()), _bits(spec))
    # acceleration_search at a = 0 alone is periodicity_search, column for column
    for kw in (dict(sigma=3.0), dict(sigma=3.0, sift=False, nharm=8, fmin=5.0, fmax=100.0)):
        ref = pe.periodicity_search(x, dt, **kw)
        got = pe.acceleration_search(x, dt, accels=[0.0], **kw)
        assert len(ref) > 10
        assert [c for c in got.colnames if c != "accel"] == ref.colnames
        assert all(np.array_equal(got[c], ref[c]) for c in ref.colnames) and np.all(got["accel"] == 0.0)
    # amax builds the grid from fmax and nharm; a 1-D float64 series is one row
    tab = pe.acceleration_search(x[0].astype(np.float64), dt, amax=3.9e5, fmax=30.0, nharm=8, sigma=8)
    grid = pe.acceleration_grid(3.9e5, n * dt, 8 * 30.0)
    assert len(tab) >= 1 and np.all(tab["row"] == 0) and np.all(np.isin(tab["accel"], grid))
    # (the coarser grid of 8 harmonics: the best trial is within a bin of drift at ftop, two steps)
    assert abs(tab["accel"][0] - ao.ACCEL) <= 2 * (grid[1] - grid[0]) and abs(tab["freq"][0] - ao.F0) <= 1 / (8 * n * dt)
    for call in (lambda: pe.acceleration_search(x, dt), lambda: pe.acceleration_search(x, dt, accels=[0.0], amax=1.0),
                 lambda: pe.acceleration_search(x, dt, accels=[0.0], nharm=12),
                 lambda: pe.acceleration_search(x, dt, accels=[0.0, 2 * 299792458.0 / (dt * n) * 1.01]),
                 lambda: pe.resample(x, 2 * 299792458.0 / (dt * n) * 1.01, dt),
                 lambda: pe.resample(x, float("nan"), dt),
                 lambda: pe.rfft_accel(x, [float("inf")], dt),
                 lambda: pe.rfft_accel(x, accels, dt, nfft=3000)):
        with pytest.raises(ValueError):
            call()


def test_abi_limits_on_the_device(hip):
    """The checks of tests/test_accel_cpu.py hold with real device pointers too."""
    import torch
    lib = hip.lib()
    x = torch.zeros((2, 300), dtype=torch.float32, device="cuda")
    af = torch.zeros(40000, dtype=torch.float64, device="cuda")
    spec = torch.zeros((4, 257), dtype=torch.complex64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    args = (hip.ptr(x), hip.PU_F32, 2, 300, 300, None, hip.ptr(af))
    assert lib.pu_rfft_accel(*args, 40000, 512, hip.ptr(spec), 257, hip.ptr(ws), 1 << 16, None) == -1
    assert "grid limit" in lib.pu_last_error().decode()
    assert lib.pu_rfft_accel(*args, 2, 512, hip.ptr(spec), 257, hip.ptr(ws), 16, None) == -1
    assert "workspace" in lib.pu_last_error().decode()
    assert lib.pu_rfft_accel(hip.ptr(x), hip.PU_F32, 2, 300, 299, None, hip.ptr(af), 2, 512, hip.ptr(spec), 257,
                             hip.ptr(ws), 1 << 16, None) == -1
    assert "leading dimension" in lib.pu_last_error().decode()
