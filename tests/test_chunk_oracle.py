"""tests/chunk_oracle.py (the host restatement the GPU file-path tests compare against) pinned
on the CPU: its spectra and channel mask against the goldens made by the reference's own code,
its chunk list against the geometry worked out by hand, and the tie condition the GPU tests
rely on, on the oracle's own per-width S/N."""
import numpy as np
import pytest

import chunk_oracle as ck
from pulsarutils import sigproc
from synth_files import write_stats_file


@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_spectral_stats_and_bad_chans_equal_the_goldens(golden, tmp_path, dt):
    arrays, _ = golden
    fname, _ = write_stats_file(str(tmp_path), dt)
    mean_spec, std_spec = ck.spectral_stats(fname)
    np.testing.assert_array_equal(mean_spec, arrays[f"fil_{dt}_mean"])
    np.testing.assert_array_equal(std_spec, arrays[f"fil_{dt}_std"])
    bad = ck.bad_chans(fname)
    assert bad.dtype == bool and bad.any()
    np.testing.assert_array_equal(bad, arrays[f"fil_{dt}_badchans"])


def _edges(geom):
    ftop = geom["fch1"] - 0.5 * geom["foff"]
    return ftop + geom["foff"] * ck.NCH, ftop


def test_chunk_list_main_geometry():
    """delta_delay(350, 1200, 1500) = 0.361 s = 1805 samples: step 3610, hop 1805; the chunk
    at 18050 is the 1950-sample tail, the 145 samples at 19855 are skipped."""
    fbottom, ftop = _edges(ck.MAIN)
    assert (fbottom, ftop) == (1500.0 + 150.0 / 64 - 300.0, 1500.0 + 150.0 / 64)
    step, chunks = ck.chunk_list(ck.MAIN["ns"], ck.TSAMP, fbottom, ftop, 350)
    assert step == 3610
    assert len(chunks) == 11
    assert chunks[:2] == [(0, 3610), (1805, 5415)] and chunks[-1] == (18050, 20000)
    assert chunks == [(i * 1805, min(i * 1805 + 3610, 20000)) for i in range(11)]
    assert 20000 - 11 * 1805 == 145
    # tmin skips the chunks that start before it; chunk_length sets the step
    assert ck.chunk_list(20000, ck.TSAMP, fbottom, ftop, 350, tmin=1.0)[1] == chunks[3:]
    assert chunks[3][0] * ck.TSAMP >= 1.0 > chunks[2][0] * ck.TSAMP
    step, short = ck.chunk_list(20000, ck.TSAMP, fbottom, ftop, 350, chunk_length=0.2)
    assert step == 2000 and short == [(i * 1000, i * 1000 + 2000) for i in range(19)] + [(19000, 20000)]


def test_chunk_list_positive_foff_takes_the_minimum_step():
    """foff > 0: the header's ``fbottom`` is the upper band edge, delta_delay is negative and
    the step is the floor of 128 samples; 2000 samples end in an 80-sample tail."""
    fbottom, ftop = _edges(ck.UP)
    assert fbottom > ftop
    from pulsarutils._planner import delta_delay
    assert delta_delay(350, fbottom, ftop) < 0
    step, chunks = ck.chunk_list(ck.UP["ns"], ck.TSAMP, fbottom, ftop, 350)
    assert step == 128
    assert len(chunks) == 31 and chunks[-2:] == [(1856, 1984), (1920, 2000)]
    assert {b - a for a, b in chunks} == {128, 80}


def test_header_convention_and_default_resample(tmp_path):
    """read_header gives chunk_list its band edges; the default sample time resamples the main
    geometry by N = 3, and N = rint(ratio) (2.6 -> 3, 2.4 -> 2, 1.9 -> 1)."""
    fname = str(tmp_path / "main.fil")
    ck.write_pulse_file(fname, "u8", ns=256, **{k: ck.MAIN[k] for k in ("fch1", "foff")})
    h = sigproc.read_header(fname)[0]
    assert (h["fbottom"], h["ftop"]) == _edges(ck.MAIN) and h["nsamples"] == 256
    assert ck.resample_factor(h, 250) == (3, 3 * ck.TSAMP)
    assert ck.resample_factor(h, 250, ck.TSAMP) == (1, ck.TSAMP)
    assert ck.resample_factor(h, 250, 2.6 * ck.TSAMP) == (3, 3 * ck.TSAMP)
    assert ck.resample_factor(h, 250, 2.4 * ck.TSAMP) == (2, 2 * ck.TSAMP)
    assert ck.resample_factor(h, 250, 1.9 * ck.TSAMP) == (1, 1.9 * ck.TSAMP)


@pytest.mark.parametrize("geom,N", [("UP", 1), ("UP", 3), ("MAIN", 1), ("MAIN", 3)])
def test_expected_chunks_and_tie_condition(tmp_path, geom, N):
    """expected_chunks on the oracle alone: plane shapes (the resample drops the remainder),
    the trial grid at N * tsamp, the pulse in the main geometry, and the tie condition of the
    GPU tests (at most max(2, ndm // 100) trials per chunk whose two best width S/N are within
    the comparison's tolerance of each other) at both tolerances."""
    g = getattr(ck, geom)
    fname = str(tmp_path / "f.fil")
    ck.write_pulse_file(fname, "u8", **g)
    for sdt, rtol in (("f64", 1e-9), ("f32", 1e-5)):
        exp = ck.expected_chunks(fname, 250, 350, N * ck.TSAMP, search_dtype=sdt)
        h = sigproc.read_header(fname)[0]
        assert [(e[0], e[1]) for e in exp] == ck.chunk_list(g["ns"], ck.TSAMP, h["fbottom"], h["ftop"], 350)[1]
        for istart, iend, plane, dms, (mx, sd, snr, win), wsnr in exp:
            assert plane.shape == (ck.NCH, (iend - istart) // N) and plane.dtype == np.float64
            assert np.isfinite(plane).all() and np.isfinite(wsnr).all() and np.isfinite(snr).all()
            assert ck.count_ties(wsnr, rtol).sum() <= max(2, dms.size // 100)
        if geom == "MAIN":
            best = max(exp, key=lambda e: e[4][2].max())
            assert best[0] <= ck.PULSE_T < best[1]
            assert abs(best[3][np.argmax(best[4][2])] - ck.PULSE_DM) < 3
    if geom == "UP":
        assert {e[2].shape[1] for e in exp} == ({128, 80} if N == 1 else {42, 26})
