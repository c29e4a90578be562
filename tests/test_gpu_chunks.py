"""clean.search_by_chunks, EVERY chunk against the host restatement (tests/chunk_oracle.py,
pinned by tests/test_chunk_oracle.py): the chunk list, the cleaned (flipped, resampled) plane
of the candidate pickle bit for bit, the trial grid and the search table at SURVEY §8a's bars -
overlapped (loader thread + copy stream) and profiled (synchronised), N = 1 and 3, float64 and
float32 search, 8-bit / 16-bit / float32 files, the 128-sample minimum step of a foff > 0 file
and the driver's options.  Plus the 16-bit file through get_spectral_stats / get_bad_chans and
cleanup_data."""
import pickle

import numpy as np
import pytest

import chunk_oracle as ck
from pulsarutils import clean, sigproc, stats
from test_gpu_cleanup import data_bytes, expected_rows, levels

pytestmark = pytest.mark.gpu

DMMIN, DMMAX = 250, 350
RTOL = {"f64": 1e-9, "f32": 1e-5}
SAMPLE_TIMES = {"N1": ck.TSAMP, "N3": 3 * ck.TSAMP, "default": None}


@pytest.fixture(scope="module")
def files(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("chunks")
    out = {}
    for kind in ("u8", "u16", "f32"):
        out[kind] = str(d / f"main_{kind}.fil")
        ck.write_pulse_file(out[kind], kind, **ck.MAIN)
    out["up"] = str(d / "up_u8.fil")
    ck.write_pulse_file(out["up"], "u8", **ck.UP)
    return out


_EXPECTED = {}


def expected(fname, **kw):
    """chunk_oracle.expected_chunks, computed once per configuration and left unchanged."""
    key = (fname,) + tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))
    if key not in _EXPECTED:
        _EXPECTED[key] = ck.expected_chunks(fname, DMMIN, DMMAX, **kw)
    return _EXPECTED[key]


def run(fname, workdir, monkeypatch, profile=None, **kw):
    """search_by_chunks with every searched chunk returned as a candidate, and its pickle."""
    workdir.mkdir()
    monkeypatch.chdir(workdir)
    cands = clean.search_by_chunks(fname, dmmin=DMMIN, dmmax=DMMAX, snr_threshold=-np.inf, save_candidates=True,
                                   profile=profile, **kw)
    root = fname.rsplit("/", 1)[-1].split(".")[0]
    for c in cands:
        with open(workdir / f"{root}_{c['istart']}-{c['iend']}.pkl", "rb") as fh:
            c["info"] = pickle.load(fh)
    return cands


def check(cands, exp, fname, search_dtype, N, pulse):
    h = sigproc.read_header(fname)[0]
    rtol = RTOL[search_dtype]
    np.testing.assert_array_equal(np.loadtxt(fname + ".badchans").astype(bool), ck.bad_chans(fname))
    assert [(c["istart"], c["iend"]) for c in cands] == [(e[0], e[1]) for e in exp]
    for c, (istart, iend, plane, dms, (omx, osd, osnr, owin), wsnr) in zip(cands, exp):
        where = f"chunk {istart}-{iend}"
        info, tab = c["info"], c["table"]
        assert plane.shape[1] == (iend - istart) // N, where
        assert info.allprofs.dtype == np.float64 and info.allprofs.shape == plane.shape, where
        assert np.array_equal(info.allprofs, plane), (where, np.argwhere(info.allprofs != plane)[:5])
        assert (info.nbin, info.nchan) == (plane.shape[1], plane.shape[0]), where
        assert info.pulse_freq == 1 / (plane.shape[1] * (N * h["tsamp"])), where
        assert (info.start_freq, info.bandwidth) == (h["fbottom"], h["bandwidth"]), where
        np.testing.assert_array_equal(tab["DM"], dms, err_msg=where)
        for col, want in (("max", omx), ("std", osd), ("snr", osnr)):
            got = np.asarray(tab[col])
            print(f"{where} {col}: max rel err {np.max(np.abs(got - want) / np.abs(want)):.3e}")
            np.testing.assert_allclose(got, want, rtol=rtol, atol=0, err_msg=f"{where} {col}")
        tie = ck.count_ties(wsnr, rtol)
        assert tie.sum() <= max(2, dms.size // 100), (where, int(tie.sum()))
        win = np.asarray(tab["rebin"])
        assert np.array_equal(win[~tie], owin[~tie]), (where, np.nonzero((win != owin) & ~tie)[0][:10])
        assert c["t0"] == istart * h["tsamp"] and c["dm"] == dms[np.argmax(tab["snr"])], where
    if pulse:
        best = max(cands, key=lambda c: c["snr"])
        assert abs(best["dm"] - ck.PULSE_DM) < 3 and best["istart"] <= ck.PULSE_T < best["iend"]


def assert_same_runs(a, b):
    """Two runs of the driver bit-equal: every table column and every pickled plane."""
    assert [(c["istart"], c["iend"]) for c in a] == [(c["istart"], c["iend"]) for c in b]
    for ca, cb in zip(a, b):
        for col in ("DM", "max", "std", "snr", "rebin"):
            assert np.array_equal(np.asarray(ca["table"][col]), np.asarray(cb["table"][col])), (ca["istart"], col)
        assert np.array_equal(ca["info"].allprofs, cb["info"].allprofs), ca["istart"]


def both_ways(fname, tmp_path, monkeypatch, search_dtype, N, pulse, **kw):
    """Overlapped and profiled, each against the oracle, and bit-equal to each other."""
    exp = expected(fname, search_dtype=search_dtype, **kw)
    over = run(fname, tmp_path / "overlapped", monkeypatch, search_dtype=search_dtype, **kw)
    check(over, exp, fname, search_dtype, N, pulse)
    prof = []
    sync = run(fname, tmp_path / "profiled", monkeypatch, profile=prof, search_dtype=search_dtype, **kw)
    assert [(p["istart"], p["istart"] + p["nsamples"]) for p in prof] == [(e[0], e[1]) for e in exp]
    check(sync, exp, fname, search_dtype, N, pulse)
    assert_same_runs(over, sync)
    return exp


@pytest.mark.parametrize("search_dtype", ["f64", "f32"])
@pytest.mark.parametrize("resample", ["N1", "N3", "default"])
def test_every_chunk_main(files, tmp_path, monkeypatch, resample, search_dtype):
    """The main geometry: 11 chunks of 3610 samples and a 1950-sample tail (a plan rebuild);
    neither is a multiple of 3, so the N = 3 resample drops a remainder.  The default sample
    time gives N = 3 here."""
    N = 1 if resample == "N1" else 3
    assert ck.resample_factor(sigproc.read_header(files["u8"])[0], DMMIN, SAMPLE_TIMES[resample])[0] == N
    exp = both_ways(files["u8"], tmp_path, monkeypatch, search_dtype, N, True,
                    new_sample_time=SAMPLE_TIMES[resample])
    assert len(exp) == 11 and (exp[-1][0], exp[-1][1]) == (18050, 20000)
    assert {e[2].shape[1] for e in exp} == {3610 // N, 1950 // N}


@pytest.mark.parametrize("kind,resample,search_dtype", [("u16", "N1", "f64"), ("u16", "default", "f32"),
                                                         ("f32", "N1", "f32"), ("f32", "default", "f64")])
def test_every_chunk_16bit_and_float32_files(files, tmp_path, monkeypatch, kind, resample, search_dtype):
    """A 16-bit file (samples up to 51000: converted to float64 on the device) and a float32
    file through the overlapped driver."""
    fname = files[kind]
    fil = sigproc.FilReader(fname)
    assert fil.nbits == {"u16": 16, "f32": 32}[kind]
    assert fil.dtype == {"u16": np.uint16, "f32": np.float32}[kind] and (kind == "f32" or fil.readBlock(0, 64).max() > 255)
    N = 1 if resample == "N1" else 3
    exp = expected(fname, search_dtype=search_dtype, new_sample_time=SAMPLE_TIMES[resample])
    got = run(fname, tmp_path / "run", monkeypatch, search_dtype=search_dtype, new_sample_time=SAMPLE_TIMES[resample])
    check(got, exp, fname, search_dtype, N, True)
    assert len(exp) == 11


@pytest.mark.parametrize("search_dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [1, 3])
def test_every_chunk_minimum_step(files, tmp_path, monkeypatch, N, search_dtype):
    """foff > 0 (no band flip; the header's ``fbottom`` is the upper edge, so the whole-band
    delay is negative and the step is the floor of 128): 30 chunks of 128 samples and an
    80-sample tail, cleaned at n = 128 and 80, searched at nbin 128 / 80 (N = 1) or 42 / 26
    (N = 3), with a plan rebuild for the tail.

    These series are one partial time tile of the search kernel.  With that tile's sums shifted
    by its first sample the float32 search missed the 1e-5 bar at nbin 42 (width 8, 5 windows:
    S/N 5.8e-5 off in chunk 512-640, four trials above 1e-5 in the file; max and std within
    1.2e-6); shifted by the tile's mean (dedisp_common.h write_outputs) it holds."""
    exp = both_ways(files["up"], tmp_path, monkeypatch, search_dtype, N, False, new_sample_time=N * ck.TSAMP)
    assert len(exp) == 31 and (exp[-1][0], exp[-1][1]) == (1920, 2000)
    assert [e[2].shape[1] for e in exp] == [128 // N] * 30 + [80 // N]


@pytest.mark.parametrize("option", [dict(tmin=1.0), dict(surelybad=[5, 40]), dict(zero_dm=True),
                                    dict(chunk_length=0.2)], ids=lambda o: next(iter(o)))
def test_every_chunk_options(files, tmp_path, monkeypatch, option):
    fname = files["u8"]
    exp = expected(fname, search_dtype="f64", new_sample_time=ck.TSAMP, **option)
    got = run(fname, tmp_path / "run", monkeypatch, search_dtype="f64", new_sample_time=ck.TSAMP, **option)
    check(got, exp, fname, "f64", 1, True)
    if "tmin" in option:
        assert len(exp) == 8 and exp[0][0] == 5415
    if "surelybad" in option:   # the flipped plane: file channel c is row 63 - c
        assert all(not c["info"].allprofs[[63 - 5, 63 - 40]].any() and c["info"].allprofs[0].any() for c in got)
    if "zero_dm" in option:
        plain = expected(fname, search_dtype="f64", new_sample_time=ck.TSAMP)
        assert not np.array_equal(plain[0][2], exp[0][2])
    if "chunk_length" in option:
        assert len(exp) == 20 and (exp[-1][0], exp[-1][1]) == (19000, 20000)


# ------------------------------------------------------------------ 16-bit files

@pytest.mark.parametrize("ns", [25000, 10000, 9999])
def test_spectral_stats_16bit(gpu, tmp_path, ns):
    """get_spectral_stats / get_bad_chans of a 16-bit file (values above 255) bit-equal to the
    host restatement: more than two chunks with a short last one, exactly one chunk, and a
    file shorter than one chunk."""
    from synth_files import stats_file_data
    x = stats_file_data("u8")[:ns].astype(np.uint16) * np.uint16(200)
    fname = str(tmp_path / "syn_u16.fil")
    sigproc.write_filterbank(fname, x, fch1=1500.0, foff=-300.0 / x.shape[1], tsamp=64e-6)
    assert sigproc.FilReader(fname).nbits == 16 and x.max() > 255
    want_mean, want_std = ck.spectral_stats(fname)
    mean_spec, std_spec = stats.get_spectral_stats(fname)
    np.testing.assert_array_equal(mean_spec, want_mean)
    np.testing.assert_array_equal(std_spec, want_std)
    want_bad = ck.bad_chans(fname)
    assert want_bad.any() and not want_bad.all()
    np.testing.assert_array_equal(stats.get_bad_chans(fname), want_bad)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_cleanup_16bit_and_float32_input(files, tmp_path, kind):
    """cleanup_data of a 16-bit and of a float32 file to 8 bits: the output bytes equal the
    host composition test_gpu_cleanup.py uses for 8-bit input (oracle renormalize -> the
    numpy quantisation), chunk by chunk."""
    fname = files[kind]
    x = sigproc.FilReader(fname).readBlock(0, ck.MAIN["ns"]).T
    out = str(tmp_path / "clean.fil")
    res = clean.cleanup_data(fname, out, nbits=8, chunksize=8192)
    chunks = [(0, 8192), (8192, 11808)]
    mask = ck.bad_chans(fname)
    mean_spec, std_spec = ck.spectral_stats(fname)
    scale, offset = levels(8, mask, mean_spec, std_spec)
    assert res["nchunks"] == 2 and res["nsamples"] == ck.MAIN["ns"]
    np.testing.assert_array_equal(res["mask"], mask)
    np.testing.assert_array_equal(res["scale"], scale)
    hdr, got = data_bytes(out)
    assert hdr["nbits"] == 8 and hdr["nsamples"] == ck.MAIN["ns"]
    np.testing.assert_array_equal(got, expected_rows(x, chunks, mask, scale, offset, 8))
