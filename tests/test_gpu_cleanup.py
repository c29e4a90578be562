"""clean.cleanup_data: the cleaned file's bytes against the composition of the reference
steps (oracle renormalize -> the numpy quantisation of include/pulsarutils_hip.h -> _pack),
the overlapped writer against the synchronised one, and a dispersed pulse that survives the
clean to 8 bits and is found in the output by search_by_chunks."""
import numpy as np
import pytest

from oracle import clean_oracle as co
from pulsarutils import clean, sigproc, stats

pytestmark = pytest.mark.gpu

NCH, NS, TSAMP = 64, 20000, 2e-4
FCH1, FOFF = 1500.0, -300.0 / NCH
HOT = (9, 41)


@pytest.fixture(scope="module")
def noisy_file(gpu, tmp_path_factory):
    """A u8 file with two hot channels and a broadband spike; its mask and spectra (computed
    once, by the functions cleanup_data's docstring names)."""
    rng = np.random.default_rng(31)
    lvl = np.full(NCH, 60.0)
    lvl[list(HOT)] = 150.0
    x = rng.standard_normal((NS, NCH)) * 6 + lvl
    x[12345] += 80.0
    x = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    fname = str(tmp_path_factory.mktemp("cleanup") / "noisy.fil")
    sigproc.write_filterbank(fname, x, fch1=FCH1, foff=FOFF, tsamp=TSAMP, tstart=58000.5, source_name="B0000+00")
    mask = stats.get_bad_chans(fname)
    assert mask[list(HOT)].all() and mask.sum() < NCH // 4
    mean_spec, std_spec = stats.get_spectral_stats(fname)
    return fname, x, mask, mean_spec, std_spec


def levels(nbits, mask, mean_spec, std_spec):
    out_mean, out_sigma = {1: (0.5, 0.5), 2: (1.5, 1.0), 4: (7.5, 2.5), 8: (96.0, 16.0)}[nbits]
    sig = std_spec / mean_spec
    ok = ~mask & np.isfinite(sig) & (sig > 0)
    scale = np.zeros(mask.size)
    scale[ok] = out_sigma / sig[ok]
    return scale, np.full(mask.size, out_mean)


def expected_rows(x_tc, chunks, mask, scale, offset, nbits, **kw):
    top = (1 << nbits) - 1
    rows = []
    for a, n in chunks:
        ren = co.renormalize(np.ascontiguousarray(x_tc[a:a + n].T), badchans_mask=mask, **kw)
        v = ren * scale[:, None] + offset[:, None]
        v = np.where(np.isnan(v), offset[:, None], v)
        q = np.clip(np.rint(v), 0, top).astype(np.uint8)
        rows.append(np.ascontiguousarray(q.T) if nbits == 8 else sigproc._pack(q.T, nbits))
    return np.concatenate(rows)


def data_bytes(fname):
    hdr, hdr_len = sigproc.read_header(fname)
    return hdr, np.fromfile(fname, dtype=np.uint8, offset=hdr_len).reshape(hdr["nsamples"], -1)


@pytest.mark.parametrize("nbits,cut", [(8, False), (2, False), (8, True)])
def test_file_bytes_equal_the_composition(noisy_file, tmp_path, nbits, cut):
    fname, x, mask, mean_spec, std_spec = noisy_file
    out = str(tmp_path / "clean.fil")
    prof = []
    res = clean.cleanup_data(fname, out, nbits=nbits, chunksize=8192, cut_outliers=cut, profile=prof)
    chunks = [(0, 8192), (8192, 11808)]           # the 3616-sample tail is merged
    assert res["nchunks"] == 2 and [(p["istart"], p["nsamples"]) for p in prof] == chunks
    assert all(k in p for p in prof for k in ("h2d", "transpose", "clean", "quantize", "d2h", "write"))
    scale, offset = levels(nbits, mask, mean_spec, std_spec)
    np.testing.assert_array_equal(res["mask"], mask)
    np.testing.assert_array_equal(res["scale"], scale)
    np.testing.assert_array_equal(res["offset"], offset)
    hdr, got = data_bytes(out)
    assert hdr["nsamples"] == NS == res["nsamples"] and hdr["nbits"] == nbits == res["nbits"] and hdr["nifs"] == 1
    src_hdr = sigproc.read_header(fname)[0]
    for k in ("source_name", "tstart", "tsamp", "fch1", "foff", "nchans", "machine_id", "telescope_id",
              "data_type"):
        assert hdr[k] == src_hdr[k], k
    want = expected_rows(x, chunks, mask, scale, offset, nbits, cut_outliers=cut)
    if cut:  # the spike's bins are cut in the reference steps: the case is not vacuous
        plain = expected_rows(x, chunks, mask, scale, offset, nbits)
        assert (plain != want).any()
    np.testing.assert_array_equal(got, want)
    # masked channels are the constant rint(out_mean)
    back = sigproc.FilReader(out).readBlock(0, NS)
    const = {8: 96, 2: 2}[nbits]
    assert (back[list(HOT)] == const).all() and not (back[0] == const).all()


def test_overlapped_equals_synchronised(noisy_file, tmp_path):
    fname = noisy_file[0]
    a, b = str(tmp_path / "overlap.fil"), str(tmp_path / "sync.fil")
    ra = clean.cleanup_data(fname, a, nbits=4, chunksize=4096)
    prof = []
    rb = clean.cleanup_data(fname, b, nbits=4, chunksize=4096, profile=prof)
    assert ra["nchunks"] == rb["nchunks"] == len(prof) == 5
    assert ra["nsamples"] == rb["nsamples"] == NS
    assert open(a, "rb").read() == open(b, "rb").read()


def test_float32_output_is_the_renormalised_plane(noisy_file, tmp_path):
    fname, x, mask, _, _ = noisy_file
    out = str(tmp_path / "f32.fil")
    res = clean.cleanup_data(fname, out, nbits=32, chunksize=2**17)
    assert res["nchunks"] == 1 and res["scale"] is None and res["offset"] is None
    got = sigproc.FilReader(out).readBlock(0, NS)
    want = co.renormalize(np.ascontiguousarray(x.T), badchans_mask=mask).astype(np.float32)
    np.testing.assert_array_equal(got, want)


def test_pulse_survives_the_clean(gpu, tmp_path, monkeypatch):
    """The geometry of test_gpu_files.test_search_by_chunks_finds_pulse (a pulse of +40 counts
    per channel at DM 300, t = 9000) with a hot channel and a broadband spike at one sample
    added: cleaned to 8 bits with cut_outliers, then searched in the OUTPUT file.

    The reference steps alone (clean_oracle.renormalize with cut_outliers -> the numpy
    quantisation with cleanup_data's default levels -> clean_oracle.renormalize per search
    chunk -> oracle.search, run on the CPU at these amplitudes) find the pulse in chunk
    7220-10830 at DM 300.01 with S/N 39.8, a margin of 33.8 over the threshold of 6; the
    chunks that hold none of the pulse stay below 5.3."""
    from pulsarutils import _planner
    rng = np.random.default_rng(21)
    x = np.clip(np.rint(rng.standard_normal((NS, NCH)) * 6 + 60), 0, 255)
    fbottom = FCH1 - 0.5 * FOFF + FOFF * NCH
    sh = _planner.dedispersion_shifts(NCH, 300.0, fbottom, 300.0, TSAMP).astype(int)
    for c in range(NCH):
        x[(9000 + sh[c]) % NS, NCH - 1 - c] += 40
    x[:, 17] += 90
    x[4000, :] += 100
    x = np.clip(x, 0, 255).astype(np.uint8)
    fname, out = str(tmp_path / "pulse.fil"), str(tmp_path / "pulse_clean.fil")
    sigproc.write_filterbank(fname, x, fch1=FCH1, foff=FOFF, tsamp=TSAMP)
    monkeypatch.chdir(tmp_path)
    res = clean.cleanup_data(fname, out, nbits=8, cut_outliers=True)
    assert res["mask"][17] and res["nsamples"] == NS
    cands = clean.search_by_chunks(out, dmmin=250, dmmax=350, new_sample_time=TSAMP, save_candidates=False)
    assert cands, "pulse not found in the cleaned file"
    best = max(cands, key=lambda c: c["snr"])
    print(f"candidates {[(c['istart'], c['iend'], round(c['dm'], 2), round(c['snr'], 2)) for c in cands]}")
    assert abs(best["dm"] - 300) < 3 and best["istart"] <= 9000 < best["iend"]
