"""The Fourier and acceleration searches and the event extraction at the sizes their loops start to
loop: every transform length 2^8 .. 2^24, the second and third trip of the one-workgroup scans, the
grid-stride and row-batch limits, the index arithmetic of the resampling past 2^31 and on exact
ties, the tile edges of the harmonic search, and the Python batch drivers with more than one batch.

Bit for bit against tests/spectrum_oracle.py, tests/accel_oracle.py and tests/pulse_oracle.py
everywhere but the FFT, which is held to test_gpu_spectrum.py's bound against the float64 DFT.
Where a host oracle would dominate, the input is a few distinct rows (or factors) tiled: the
expectation is computed on the distinct ones and relabelled.  Every test asserts in numpy, before
the device call, that its input reaches the path it is named after."""
import math

import numpy as np
import pytest

import accel_oracle as ao
import pulse_oracle as po
import spectrum_oracle as so
import test_gpu_accel as tga
import test_gpu_pulses as tgp
import test_gpu_spectrum as tgs

pytestmark = pytest.mark.gpu

SCAN_TRIP = 8 * 1024  # entries hs_scan_kernel and event_scan_kernel take per trip


@pytest.fixture(scope="module")
def hip(gpu):
    from pulsarutils import _hip
    _hip.require_gpu()
    return _hip


# ------------------------------------------------------------------ A. every transform length

def _lg(nfft):
    return int(math.log2(nfft))


def _n2(nfft):
    """Columns of the four-step's N1 x N2 split of the nfft / 2 packed samples (one pass: all)."""
    lm = _lg(nfft) - 1
    return 1 << (lm if lm <= 12 else lm - lm // 2)


def _held(hip, x, nfft, mean, what):
    """The rows' error ratios, printed, and held to the bound."""
    n = x.shape[1]
    spec = tgs.gpu_rfft(hip, x, nfft, mean=mean, ld=n + 7, ld_spec=nfft // 2 + 9)
    ratio = tgs._ratios(spec, so.rfft(x, nfft, mean), nfft)
    print(f"nfft 2^{_lg(nfft)} {x.dtype.name} n {n} {what}: ratio {np.round(ratio, 3).tolist()}")
    assert ratio.max() <= 8.0, (what, nfft, n, ratio)
    return ratio


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lg", range(8, 21))
def test_fft_every_length(hip, lg, dtype):
    nfft = 1 << lg
    n = nfft - 24
    x = np.stack([tgs._inputs(k, n, dtype, 31 + i) for i, k in enumerate(("gauss", "tone", "offset"))])
    mean = [0.0, 0.0, float(x[2].astype(np.float64).sum() / n)]
    _held(hip, x, nfft, mean, "gauss, tone, offset")


@pytest.mark.parametrize("lg", range(8, 21))
def test_fft_unit_impulses(hip, lg):
    """One sample set: every bin has magnitude 1, so a sample read from (or a column written to) the
    wrong place moves the whole row's error to sqrt 2 of the norm.  Even and odd halves of a packed
    pair, the last and the first column of the four-step's split, the middle, the last sample."""
    nfft = 1 << lg
    n = nfft - 24
    at = [0, 1, _n2(nfft) - 1, _n2(nfft), nfft // 2, n - 1]
    x = np.zeros((len(at), n), np.float32)
    x[np.arange(len(at)), at] = 1.0
    _held(hip, x, nfft, None, f"impulses at {at}")


@pytest.mark.parametrize("lg", range(21, 25))
def test_fft_longest_lengths(hip, lg):
    """2^24: C = 4 columns and R = 2 rows per workgroup, and the first pass's twiddle exponent
    2 j2 k1 reaches nfft - 2."""
    nfft = 1 << lg
    n = nfft - 24
    x = tgs._inputs("offset", n, np.float32, lg)[None]
    _held(hip, x, nfft, [float(x[0].astype(np.float64).sum() / n)], "offset")


@pytest.mark.parametrize("lg", [8, 13, 14])
def test_fft_short_rows(hip, lg):
    """2^13: the longest single pass; 2^14: the shortest four-step.  The offset row's mean is a
    given 100 (the row's own would leave nothing of one sample)."""
    nfft = 1 << lg
    for dtype in (np.float32, np.float64):
        for n in (1, 2, nfft // 2, nfft // 2 + 1):
            x = np.stack([tgs._inputs("gauss", n, dtype, 7), tgs._inputs("offset", n, dtype, 8)])
            _held(hip, x, nfft, [0.0, 100.0], "gauss, offset - 100")
        # no samples at all: nothing to scale an error by, and nothing but zeros to transform (an
        # empty tensor has no address to pass: n = 0 of rows of NaN)
        import torch
        xd = torch.from_numpy(np.full((2, 7), np.nan, dtype)).cuda()
        md = torch.tensor([0.0, 3.0], dtype=torch.float64, device="cuda")
        spec = torch.full((2, nfft // 2 + 9), float("nan"), dtype=torch.complex64, device="cuda")
        lib = hip.lib()
        ws, wp, wsb = hip.workspace(lib.pu_rfft_workspace_bytes(2, nfft), xd.device)
        hip.check(lib.pu_rfft(hip.ptr(xd), hip.dtype_code(xd.dtype), 2, 0, 7, hip.ptr(md), nfft, hip.ptr(spec),
                              spec.stride(0), wp, wsb, hip.stream_ptr()), "pu_rfft")
        torch.cuda.synchronize()
        spec = spec.cpu().numpy()
        assert np.all(spec[:, :nfft // 2 + 1] == 0) and np.all(np.isnan(spec[:, nfft // 2 + 1:]))


# ------------------------------------------------------------------ B. the acceleration map at scale

def _indices(n, af, product=np.float64, rnd=np.rint):
    """accel_oracle.resample_indices with the product formed in ``product`` and rounded by ``rnd``:
    what a kernel with that arithmetic would read."""
    i = np.arange(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        q = (product(af) * (i * (i - n)).astype(product)).astype(np.float64)
        s = np.fmin(np.fmax(rnd(q), -i.astype(np.float64)), (n - 1 - i).astype(np.float64))
    return i + s.astype(np.int64)


def _half_away(q):
    return np.copysign(np.floor(np.abs(q) + 0.5), q)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gather_past_2_31(hip, dtype):
    n = 131075
    afac = [0.0, 0.5 / n, -0.5 / n, 2.0 ** -18, -2.0 ** -18, 2e-3, float("nan")]
    x = np.random.default_rng(n).standard_normal((2, n)).astype(dtype)
    i = np.arange(n, dtype=np.int64)
    p = i * (i - n)
    assert np.abs(p).max() > 2 ** 31
    want = np.concatenate([ao.resample(x, af) for af in afac])
    # a 32-bit product, or a float32 one, reads other samples (and other values) at af = 0.5 / n
    wrapped = p.astype(np.int32).astype(np.float64)
    with np.errstate(all="ignore"):
        s32 = np.fmin(np.fmax(np.rint(afac[1] * wrapped), -i.astype(np.float64)), (n - 1 - i).astype(np.float64))
    assert not np.array_equal(x[:, i + s32.astype(np.int64)], want[2:4])
    single = _indices(n, afac[1], product=np.float32)
    moved = int(np.sum(single != ao.resample_indices(n, afac[1])))
    print(f"n {n}: a float32 product moves {moved} indices at af = 0.5 / n")
    assert moved > 0 and not np.array_equal(x[:, single], want[2:4])
    got, gaps = tga.gpu_resample(hip, x, afac)
    assert np.all(np.isnan(gaps))
    assert got.dtype == want.dtype and got.shape == want.shape == (14, n)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gather_ties_go_to_even(hip, dtype):
    n = 257
    afac = [2.0 ** -9, -2.0 ** -9]
    x = np.random.default_rng(9).standard_normal((3, n)).astype(dtype)
    want = np.concatenate([ao.resample(x, af) for af in afac])
    i = np.arange(n, dtype=np.int64)
    for a, af in enumerate(afac):
        q = af * (i * (i - n)).astype(np.float64)
        even, away = ao.resample_indices(n, af), _indices(n, af, rnd=_half_away)
        unclamped = (np.rint(q) >= -i) & (np.rint(q) <= n - 1 - i) & (_half_away(q) >= -i) & (_half_away(q) <= n - 1 - i)
        differ = np.flatnonzero(unclamped & (even != away))
        assert differ.size >= 1 and np.all(np.abs(q[differ]) % 1.0 == 0.5), (af, differ)
        assert not np.array_equal(x[:, away], want[3 * a:3 * a + 3])
    got, gaps = tga.gpu_resample(hip, x, afac)
    assert np.all(np.isnan(gaps)) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nfft, n, rows", [(2 ** 18, 131075, 3), (2 ** 20, 2 ** 20 - 24, 1)])
def test_fused_transform_of_long_rows(hip, nfft, n, rows, dtype):
    """test_gpu_accel.py's fused-against-two-step comparison where i (i - n) passes 2^31 (2^18: the
    four-step with N1 < N2; 2^20: the production length)."""
    x, mean = tga._series(n, dtype, nfft + n)
    x, mean = np.ascontiguousarray(x[:rows]), mean[:rows]
    assert n * n // 4 > 2 ** 31
    afac = [0.0, 0.5 / n, -0.5 / n]
    fused = tga.gpu_rfft(hip, x, nfft, mean, afac=afac)
    assert fused.shape == (3 * rows, nfft // 2 + 1) and np.all(np.isfinite(fused.view(np.float32)))
    gathered, _ = tga.gpu_resample(hip, x, afac)
    assert np.array_equal(gathered, np.concatenate([ao.resample(x, af) for af in afac]))
    two_step = tga.gpu_rfft(hip, np.ascontiguousarray(gathered), nfft, np.tile(mean, 3), ld=n + 2, ld_spec=nfft // 2 + 1)
    bits = tga._bits
    assert np.array_equal(bits(fused), bits(two_step))
    assert not np.array_equal(bits(fused[:rows]), bits(fused[rows:2 * rows]))
    assert not np.array_equal(bits(fused[rows:2 * rows]), bits(fused[2 * rows:]))
    assert np.array_equal(bits(fused[:rows]), bits(tga.gpu_rfft(hip, x, nfft, mean)))  # af = 0 is pu_rfft
    r = rows - 1
    alone = tga.gpu_rfft(hip, x[r:r + 1], nfft, mean[r:r + 1], afac=afac[2:], ld=n + 64, ld_spec=nfft // 2 + 9)
    assert np.array_equal(bits(alone), bits(fused[2 * rows + r:2 * rows + r + 1]))


def test_gather_strides_the_grid(hip):
    """nacc x rows = 65538 virtual rows on a grid of 65535: the last three are written by the
    stride loop's second turn.  Their factor (a = 21845, the sixth of the seven) is not the first
    turn's."""
    rows, nacc, n = 3, 21846, 40
    distinct = np.array([0.0, 0.5 / n, -0.5 / n, 0.9 / n, -0.9 / n, 0.3 / n, float("nan")])
    afac = np.tile(distinct, nacc // distinct.size + 1)[:nacc]
    assert rows * nacc > 65535 and (rows * nacc - 1) // rows % distinct.size != 0
    x = np.random.default_rng(40).standard_normal((rows, n)).astype(np.float32)
    each = np.stack([ao.resample(x, af) for af in distinct])          # (7, rows, n)
    assert len({e.tobytes() for e in each}) == distinct.size
    want = each[np.arange(nacc) % distinct.size].reshape(nacc * rows, n)
    got, gaps = tga.gpu_resample(hip, x, afac)
    assert np.all(np.isnan(gaps)) and got.shape == want.shape
    assert got[65535:].tobytes() == want[65535:].tobytes()
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------ C. the harmonic search

def _device_norm(norm, ld):
    """A float32 (rows, nb) spectrum as a device view of leading dimension ``ld``, the gap NaN."""
    import torch
    rows, nb = norm.shape
    buf = torch.full((rows, ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :nb] = torch.from_numpy(norm).cuda()
    return buf[:, :nb]


def _slots(rec, nlev, nb):
    """The (row, level, tile) slot of each candidate record: its place in the scan."""
    ntile = (nb + 1023) // 1024
    return (rec["row"].astype(np.int64) * nlev + rec["level"]) * ntile + rec["bin"] // 1024


def _searched(hip, norm, ld, nlev, thr, caps=()):
    """The search of ``norm`` against the oracle's sums and records: with the sums written and room
    for all, fused (no sums), counting only, and at every cap of ``caps``.  Returns the records."""
    import torch
    rows, nb = norm.shape
    kmin, kmax = np.zeros(nlev, np.int64), np.full(nlev, nb, np.int64)
    want_sums = so.harmonic_sums(norm, nlev)
    want = so.candidates(want_sums, thr, kmin, kmax)
    norm_d = _device_norm(norm, ld)
    sums_d = torch.full((nlev, rows, nb), float("nan"), dtype=torch.float32, device="cuda")
    rec, count = tgs._search(hip, norm_d, nlev, thr, kmin, kmax, sums=sums_d, cap=want.size + 5)
    assert tgs._eq(sums_d.cpu().numpy(), want_sums)
    assert count == want.size and rec.size == want.size and rec.tobytes() == want.tobytes()
    rec2, count2 = tgs._search(hip, norm_d, nlev, thr, kmin, kmax, cap=want.size)
    assert count2 == want.size and rec2.tobytes() == want.tobytes()
    rec0, count0 = tgs._search(hip, norm_d, nlev, thr, kmin, kmax, cap=0)
    assert rec0.size == 0 and count0 == want.size
    for cap in caps(want) if callable(caps) else caps:
        recc, countc = tgs._search(hip, norm_d, nlev, thr, kmin, kmax, cap=cap)
        assert countc == want.size and recc.tobytes() == want[:cap].tobytes(), cap
    return want


def test_harmonic_search_scan_takes_three_trips(hip):
    from pulsarutils import periodicity as pe
    rows, nb, ld, nlev = 1500, 1100, 1104, 6
    norm = np.random.default_rng(15).standard_exponential((rows, nb)).astype(np.float32)
    norm[700, 300] = np.nan
    norm[701] = 0.0
    thr = np.array([pe.power_threshold(pe.logp_from_sigma(2.0), 1 << lv) for lv in range(nlev)], np.float32)
    assert 2 * SCAN_TRIP < rows * nlev * 2 <= 3 * SCAN_TRIP

    def caps(want):
        slot = _slots(want, nlev, nb)
        per_trip = np.bincount(slot // SCAN_TRIP, minlength=3)
        print(f"{want.size} candidates, per trip of the scan {per_trip.tolist()}")
        assert np.any(slot < SCAN_TRIP) and np.any(slot >= 2 * SCAN_TRIP) and per_trip.min() > 100
        assert not np.any(want["row"] == 701) and np.any(want["row"] == 700) and np.any(want["row"] == rows - 1)
        half = want.size // 2
        assert slot[half - 1] == slot[half] >= SCAN_TRIP  # the cap ends inside a tile of the second trip
        return [half]

    _searched(hip, norm, ld, nlev, thr, caps)


@pytest.mark.parametrize("nb", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_harmonic_search_any_number_of_bins(hip, nb):
    """A partial last tile (of one bin at 1025 and 2049), fewer bins than a wave, one bin.  The
    threshold -1 lets every local maximum through, the row's ends included."""
    nlev = 6
    norm = np.random.default_rng(nb).standard_exponential((3, nb)).astype(np.float32)
    norm[0, 0] = norm[1, nb - 1] = 30.0  # a peak on either end of a row
    want = _searched(hip, norm, nb + 3, nlev, np.full(nlev, -1.0, np.float32), caps=lambda w: [w.size // 2])
    assert np.all(np.bincount(want["level"], minlength=nlev) >= 3)  # at least one per row and level
    assert nb < 3 or (np.any(want["bin"] == 0) and np.any(want["bin"] == nb - 1))


def test_harmonic_search_peaks_and_plateaus_on_tile_edges(hip):
    """Level 0 of zeros with single peaks on both sides of the tile edge 1023|1024 and at the row's
    ends, and two-bin plateaus across 1023|1024 and 2047|2048: above the left neighbour and not
    below the right one, so a plateau's first bin is its candidate."""
    nb, ld = 2500, 2511
    norm = np.zeros((4, nb), np.float32)
    norm[0, [0, 1023, nb - 1]] = 2.0
    norm[1, 1024] = 2.0
    norm[2, [1023, 1024, 2047, 2048]] = 2.0
    norm[3, [1022, 1023]] = 2.0       # a plateau that ends on the edge, one that starts on it
    norm[3, [2048, 2049]] = 2.0
    want = _searched(hip, norm, ld, 1, np.array([0.5], np.float32), caps=[3])
    assert [(int(e["row"]), int(e["bin"])) for e in want] == [(0, 0), (0, 1023), (0, nb - 1), (1, 1024), (2, 1023),
                                                            (2, 2047), (3, 1022), (3, 2048)]
    # with the harmonics summed on top (sums of exact small integers: the same rule at every level)
    _searched(hip, norm, ld, 6, np.full(6, 0.5, np.float32))


# ------------------------------------------------------------------ D. events

DISTINCT = 41  # rows of distinct content; 41 is coprime to every block and batch size here


def _event_rows(n, seed):
    """(DISTINCT, n) float64: noise with one to three spikes per row, a row of zeros, a row with a NaN."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((DISTINCT, n))
    for r in range(DISTINCT):
        d[r, rng.choice(n, 1 + r % 3, replace=False)] += 12.0
    d[5] = 0.0
    d[11, n // 2] = np.nan
    return d


def _tiled_events(distinct, rows, threshold, labels):
    """po.events_of of the distinct rows tiled to ``rows`` rows, row r labelled ``labels[r]``."""
    each = [po.series_events(d, threshold) for d in distinct]
    assert len(each[5]) == 0 and len(each[11]) == 0 and sum(len(e) > 0 for e in each) > DISTINCT // 2
    assert len({len(e) for e in each}) >= 3  # the counts vary: an offset that slips shows
    parts = []
    for r in range(rows):
        e = each[r % DISTINCT].copy()
        e["row"] = labels[r]
        parts.append(e)
    return np.concatenate(parts), np.cumsum([len(p) for p in parts])


def test_series_events_scan_takes_three_trips(gpu):
    rows, n, thr = 4200, 64, 3.0
    assert 2 * SCAN_TRIP < rows * 4 <= 3 * SCAN_TRIP  # one block per row and window
    distinct = _event_rows(n, 64)
    index = ((np.arange(rows) * 7 + 3) % 100003).astype(np.int32)
    want, upto = _tiled_events(distinct, rows, thr, index)
    # events of the first and of the last trip (rows below 2048 and from 4096 on)
    assert upto[2047] > 1000 and upto[-1] - upto[4095] > 50
    series = tgp.padded(gpu, distinct[np.arange(rows) % DISTINCT])
    count, got = tgp.raw_events(series, thr, len(want) + 3, index=index)
    assert count == len(want)
    tgp.assert_events_equal(got[:count], want, "three trips")
    assert not got[count:].tobytes().strip(b"\0")


@pytest.mark.parametrize("with_index", [False, True])
def test_series_events_splits_at_the_row_limit(gpu, with_index):
    """33000 rows in a workspace sized for all of them: the library itself splits at 32768, carries
    the count across and labels the second batch's rows from 32768 on."""
    rows, n, thr = 33000, 16, 2.0
    distinct = _event_rows(n, 16)
    index = ((np.arange(rows) * 5 + 1) % 200003).astype(np.int32) if with_index else None
    want, upto = _tiled_events(distinct, rows, thr, index if with_index else np.arange(rows))
    first = int(upto[32767])
    assert first > 10000 and len(want) - first > 100
    series = tgp.padded(gpu, distinct[np.arange(rows) % DISTINCT], pad=3)
    count, got = tgp.raw_events(series, thr, len(want) + 3, index=index)
    assert count == len(want)
    tgp.assert_events_equal(got[:count], want, "two batches")
    assert not got[count:].tobytes().strip(b"\0")  # nothing written past the count
    # a capacity that ends inside the second batch
    cap = first + (len(want) - first) // 2
    count, got = tgp.raw_events(series, thr, cap, index=index)
    assert count == len(want)
    tgp.assert_events_equal(got, want[:cap], "cap inside the second batch")
    count, _ = tgp.raw_events(series, thr, 0, index=index, null_events=True)
    assert count == len(want)


# ------------------------------------------------------------------ E. the batch drivers

@pytest.fixture(scope="module")
def five_rows():
    """accel_oracle's drifting pulse train and its noise row, two more noise rows and a steady
    pulse train in row 3: what is found depends on the row."""
    rng = np.random.default_rng(77)
    more = rng.standard_normal((3, ao.N)).astype(np.float32)
    more[1, (np.arange(ao.N) * ao.DT * 31.3) % 1.0 < 0.05] += np.float32(1.0)
    x = np.concatenate([ao.drifting_rows(), more])
    x.setflags(write=False)
    return x


ACCELS = np.array([-3.8e5, -1.9e5, 0.0, 1.9e5, 3.8e5])
PER_ROW = 2 ** 13 * 8  # bytes of pu_rfft's workspace per row of 2^14 samples


@pytest.fixture(scope="module")
def unbatched(hip, five_rows):
    from pulsarutils import periodicity as pe
    x = five_rows
    assert pe._rows_per_call(5, ao.N) == 5 and pe._accel_batches(5, 5, ao.N) == [(0, 5, 0, 5)]
    return _driver_results(pe, x)


def _driver_results(pe, x):
    norm = pe.power_spectrum(x, block=128)
    out = {"rfft": pe.rfft(x), "power_spectrum": norm, "harmonic_sums": pe.harmonic_sums(norm, nharm=8),
           "rfft_accel": pe.rfft_accel(x, ACCELS, ao.DT)}
    for sift in (False, True):
        out["periodicity_search", sift] = pe.periodicity_search(x, ao.DT, sigma=3.0, sift=sift)
        out["acceleration_search", sift] = pe.acceleration_search(x, ao.DT, accels=ACCELS, sigma=3.0, sift=sift)
    return out


@pytest.mark.parametrize("limits, row_batches, accel_batches", [
    # two rows of workspace: rows go 2 + 2 + 1, and so does each acceleration on its own
    (dict(_FFT_WS_BYTES=2 * PER_ROW), [2, 2, 1], [(a, a + 1, r0, min(r0 + 2, 5)) for a in range(5) for r0 in (0, 2, 4)]),
    # the same from the row limit, which the normalisation and the harmonic sums loop over too
    (dict(_MAX_ROWS=2), [2, 2, 1], [(a, a + 1, r0, min(r0 + 2, 5)) for a in range(5) for r0 in (0, 2, 4)]),
    # room for ten pairs: whole accelerations, two per call
    (dict(_FFT_WS_BYTES=10 * PER_ROW), [5], [(0, 2, 0, 5), (2, 4, 0, 5), (4, 5, 0, 5)]),
])
def test_batch_drivers_label_rows_and_accelerations(hip, five_rows, unbatched, monkeypatch, limits, row_batches,
                                                    accel_batches):
    from pulsarutils import periodicity as pe
    x = five_rows
    assert hip.lib().pu_rfft_workspace_bytes(2, ao.N) - hip.lib().pu_rfft_workspace_bytes(1, ao.N) == PER_ROW
    # the unbatched answer has something to mislabel: candidates of every row, at every acceleration,
    # and the two pulse trains where they are
    ref = unbatched["acceleration_search", False]
    assert set(np.asarray(ref["row"]).tolist()) == set(range(5)) and set(np.asarray(ref["accel"]).tolist()) == set(ACCELS)
    assert (ref["row"][0], ref["accel"][0]) == (0, 3.8e5)
    assert unbatched["periodicity_search", True]["row"][0] == 3
    for name, value in limits.items():
        monkeypatch.setattr(pe, name, value)
    per = pe._rows_per_call(5, ao.N)
    assert [min(per, 5 - r0) for r0 in range(0, 5, per)] == row_batches
    assert pe._accel_batches(5, 5, ao.N) == accel_batches
    got = _driver_results(pe, x)
    for key, want in unbatched.items():
        if isinstance(want, np.ndarray):
            assert got[key].dtype == want.dtype and got[key].shape == want.shape, key
            assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint32),
                                  np.ascontiguousarray(want).view(np.uint32)), key
        else:
            assert got[key].colnames == want.colnames and len(got[key]) == len(want) > 5, key
            for c in want.colnames:
                assert np.array_equal(got[key][c], want[c]), (key, c)
