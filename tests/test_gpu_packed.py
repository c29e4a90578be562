"""1-, 2- and 4-bit SIGPROC data on the GPU: pu_unpack_transpose against a numpy
restatement of the formula in include/pulsarutils_hip.h, FilReader.read_block_device
against readBlock, and get_spectral_stats / get_bad_chans / search_by_chunks on a packed
file against the same samples stored as 8-bit (bit-equal: both feed identical uint8 tensors
to the same kernels)."""
import numpy as np
import pytest

from pulsarutils import sigproc, stats

pytestmark = pytest.mark.gpu

HDR = dict(fch1=1500.0, foff=-300.0 / 64, tsamp=64e-6)
# (nsamps, nchans): a single spectrum (one byte per row at 1 bit); just past 64 samples;
# 3-byte rows at 1 bit; ragged against the 256-sample x 128-channel tile both ways; wide rows
# (several channel tiles); a prime sample count over 16 time tiles
SHAPES = [(1, 8), (65, 8), (300, 24), (777, 136), (64, 4096), (4099, 64)]
# 5-byte rows: the loads cannot be wider than a byte
CASES = [(nbits,) + s for nbits in (1, 2, 4) for s in SHAPES] + [(2, 300, 20), (1, 300, 40)]


def expected(src, nbits, nchans):
    """dst[c, t] = (src[t, c * nbits // 8] >> (c * nbits % 8)) & (2**nbits - 1), src (nsamps, >= row bytes)."""
    c = np.arange(nchans)
    return np.ascontiguousarray(((src[:, c * nbits // 8] >> (c * nbits % 8).astype(np.uint8))
                                 & np.uint8((1 << nbits) - 1)).T)


def packed_bytes(seed, nsamps, nbytes):
    return np.random.default_rng(seed).integers(0, 256, size=(nsamps, nbytes), dtype=np.uint8)


@pytest.mark.parametrize("nbits,nsamps,nchans", CASES)
def test_unpack_shapes(gpu, nbits, nsamps, nchans):
    import torch
    src = packed_bytes(nbits * 7 + nsamps, nsamps, nchans * nbits // 8)
    out = sigproc.unpack_transpose_device(torch.from_numpy(src).to(gpu), nbits, nchans)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (nchans, nsamps) and out.is_contiguous()
    np.testing.assert_array_equal(out.cpu().numpy(), expected(src, nbits, nchans))


def _raw_call(src, nbits, nsamps, nchans, ld_src, dst, ld_dst, stream=None):
    from pulsarutils import _hip
    _hip.check(_hip.lib().pu_unpack_transpose(_hip.ptr(src), nbits, nsamps, nchans, ld_src, _hip.ptr(dst), ld_dst,
                                              _hip.stream_ptr(stream)), "pu_unpack_transpose")


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_padded_ld_dst_untouched(gpu, nbits):
    import torch
    nsamps, nchans = 777, 136
    src = packed_bytes(40 + nbits, nsamps, nchans * nbits // 8)
    dst = torch.full((nchans, nsamps + 13), 0xAB, dtype=torch.uint8, device=gpu)
    _raw_call(torch.from_numpy(src).to(gpu), nbits, nsamps, nchans, src.shape[1], dst, nsamps + 13)
    got = dst.cpu().numpy()
    np.testing.assert_array_equal(got[:, :nsamps], expected(src, nbits, nchans))
    assert np.all(got[:, nsamps:] == 0xAB)


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_padded_ld_src(gpu, nbits):
    """Rows padded by 3 bytes (a view of a wider tensor): the padding holds other values
    and is not read as channels."""
    import torch
    nsamps, nchans = 777, 136
    rb = nchans * nbits // 8
    wide = packed_bytes(50 + nbits, nsamps, rb + 3)
    view = torch.from_numpy(wide).to(gpu)[:, :rb]
    assert view.stride(0) == rb + 3
    out = sigproc.unpack_transpose_device(view, nbits, nchans)
    np.testing.assert_array_equal(out.cpu().numpy(), expected(wide[:, :rb], nbits, nchans))


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_src_offset_by_one_byte(gpu, nbits):
    import torch
    nsamps, nchans = 300, 128            # 16/32/64-byte rows: only the pointer is misaligned
    rb = nchans * nbits // 8
    flat = packed_bytes(60 + nbits, 1, nsamps * rb + 1)[0]
    dev = torch.from_numpy(flat).to(gpu)
    view = dev[1:].view(nsamps, rb)
    assert view.data_ptr() % 2 == 1
    out = sigproc.unpack_transpose_device(view, nbits, nchans)
    np.testing.assert_array_equal(out.cpu().numpy(), expected(flat[1:].reshape(nsamps, rb), nbits, nchans))


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_non_default_stream(gpu, nbits):
    import torch
    nsamps, nchans = 777, 136
    src = packed_bytes(70 + nbits, nsamps, nchans * nbits // 8)
    dsrc = torch.from_numpy(src).to(gpu)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        out = sigproc.unpack_transpose_device(dsrc, nbits, nchans)
    side.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), expected(src, nbits, nchans))


def test_empty_block(gpu):
    import torch
    out = sigproc.unpack_transpose_device(torch.empty((0, 4), dtype=torch.uint8, device=gpu), 2, 16)
    assert tuple(out.shape) == (16, 0)
    with pytest.raises(ValueError, match="pu_unpack_transpose"):
        sigproc.unpack_transpose_device(torch.zeros((4, 4), dtype=torch.uint8, device=gpu), 3, 8)
    with pytest.raises(ValueError):
        sigproc.unpack_transpose_device(torch.zeros((4, 3), dtype=torch.uint8, device=gpu), 2, 16)


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_read_block_device_matches_read_block(gpu, tmp_path, nbits):
    """An interior block and the short last block; 72 channels are 9-byte rows at 1 bit.
    The 8-bit file takes the pu_transpose path through the same methods."""
    nsamps, nchans = 1000, 72
    x = np.random.default_rng(80 + nbits).integers(0, 1 << nbits, size=(nsamps, nchans)).astype(np.uint8)
    fname = str(tmp_path / "blk.fil")
    sigproc.write_filterbank(fname, x, nbits=nbits, **HDR)
    fil = sigproc.FilReader(fname)
    for start, n, want in ((137, 400, 400), (900, 400, 100)):
        host = fil.readBlock(start, n)
        dev = fil.read_block_device(start, n)
        assert tuple(dev.shape) == (nchans, want) and dev.is_contiguous()
        np.testing.assert_array_equal(host, x[start:start + want].T)
        np.testing.assert_array_equal(dev.cpu().numpy(), host)


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_stats_equal_to_8bit_file(gpu, tmp_path, nbits):
    nch, ns = 64, 25000
    top = (1 << nbits) - 1
    rng = np.random.default_rng(90 + nbits)
    lvl = np.full(nch, 0.35 * top)
    lvl[[9, 41]] = 0.8 * top             # two hot channels
    x = np.clip(np.rint(rng.standard_normal((ns, nch)) * (0.25 * top + 0.3) + lvl), 0, top).astype(np.uint8)
    packed, plain = str(tmp_path / "p.fil"), str(tmp_path / "u8.fil")
    sigproc.write_filterbank(packed, x, nbits=nbits, **HDR)
    sigproc.write_filterbank(plain, x, **HDR)
    mp, sp = stats.get_spectral_stats(packed)
    m8, s8 = stats.get_spectral_stats(plain)
    np.testing.assert_array_equal(mp, m8)
    np.testing.assert_array_equal(sp, s8)
    # and they are the statistics of the data (float64 sums of small integers are exact)
    np.testing.assert_array_equal(mp, x.sum(0, dtype=np.float64) / ns)
    bp, b8 = stats.get_bad_chans(packed), stats.get_bad_chans(plain)
    np.testing.assert_array_equal(bp, b8)
    assert bp[9] and bp[41]


@pytest.mark.parametrize("nbits,mu,sig,amp,seed", [(1, 0.5, 0.6, 1, 22), (2, 1.5, 0.8, 2, 23), (4, 7.5, 2.5, 6, 25)])
def test_search_by_chunks_packed_equals_8bit(gpu, tmp_path, monkeypatch, nbits, mu, sig, amp, seed):
    """The geometry of test_gpu_files.test_search_by_chunks_finds_pulse, quantised to nbits:
    the packed file and the 8-bit file of the same samples give the same candidate chunks
    with bit-equal tables, and the highest-S/N candidate is the pulse (several chunks pass
    the threshold, so the assertion is on the best one)."""
    from pulsarutils import clean, _planner
    nch, ns, tsamp = 64, 20000, 2e-4
    fch1, foff = 1500.0, -300.0 / nch
    top = (1 << nbits) - 1
    rng = np.random.default_rng(seed)
    x = np.clip(np.rint(rng.standard_normal((ns, nch)) * sig + mu), 0, top)
    fbottom = fch1 - 0.5 * foff + foff * nch
    sh = _planner.dedispersion_shifts(nch, 300.0, fbottom, 300.0, tsamp).astype(int)
    for c in range(nch):
        x[(9000 + sh[c]) % ns, nch - 1 - c] += amp
    x = np.clip(x, 0, top).astype(np.uint8)
    monkeypatch.chdir(tmp_path)
    cands = {}
    for name, kw in (("packed", {"nbits": nbits}), ("u8", {})):
        fname = str(tmp_path / f"pulse_{name}.fil")
        sigproc.write_filterbank(fname, x, fch1=fch1, foff=foff, tsamp=tsamp, **kw)
        cands[name] = clean.search_by_chunks(fname, dmmin=250, dmmax=350, new_sample_time=tsamp,
                                             save_candidates=False)
    assert cands["packed"], "pulse not found"
    assert [(c["istart"], c["iend"]) for c in cands["packed"]] == [(c["istart"], c["iend"]) for c in cands["u8"]]
    for cp, c8 in zip(cands["packed"], cands["u8"]):
        for col in ("max", "std", "snr", "rebin"):
            np.testing.assert_array_equal(np.asarray(cp["table"][col]), np.asarray(c8["table"][col]))
    best = max(cands["packed"], key=lambda c: c["snr"])
    print(f"nbits {nbits}: candidates {[(c['istart'], c['iend'], c['dm'], round(c['snr'], 2)) for c in cands['packed']]}")
    assert abs(best["dm"] - 300) < 3 and best["istart"] <= 9000 < best["iend"]
