"""sigproc.FilWriter: header carried through, streaming blocks read back by FilReader, the
device path equal to host packing - and write_filterbank still writing the bytes it wrote
before it shared the header builder."""
import hashlib

import numpy as np
import pytest

from pulsarutils import sigproc

HDR = dict(fch1=1500.0, foff=-300.0 / 64, tsamp=64e-6)
# SHA-256 of the files write_filterbank made, at the commit before FilWriter existed (its own
# header code, run on the input below), for np.random.default_rng(1234).integers(0, 4,
# size=(50, 16), dtype=np.uint8) with HDR and the default tstart / source_name
PARENT_SHA256 = {None: "9ed1b4477af8510cf0edd7f0e4b1a50aae44fb8edb8d6fe06e9872e01b7c4e16",
                 2: "5b0a706028e99b86cc8f0cde4987ec929574d2d0a8b224436435dc89fdadb0b6"}


@pytest.mark.parametrize("nbits", [None, 2])
def test_write_filterbank_bytes_unchanged(tmp_path, nbits):
    x = np.random.default_rng(1234).integers(0, 4, size=(50, 16), dtype=np.uint8)
    fname = str(tmp_path / "w.fil")
    sigproc.write_filterbank(fname, x, nbits=nbits, **HDR)
    assert hashlib.sha256(open(fname, "rb").read()).hexdigest() == PARENT_SHA256[nbits]


def source_header(tmp_path, nchans):
    """A FilReader.header (derived keys and all) with extra keys write_filterbank never writes."""
    src = str(tmp_path / "src.fil")
    hdr = {"source_name": "J0534+2200", "rawdatafile": "scan_0042.raw", "machine_id": 7, "telescope_id": 6,
           "data_type": 1, "barycentric": 0, "nchans": nchans, "nbits": 8, "nifs": 1, "nbeams": 1, "ibeam": 1,
           "fch1": 1500.0, "foff": -300.0 / 64, "tstart": 58849.123456789, "tsamp": 64e-6, "src_raj": 53431.9,
           "src_dej": 220052.1, "az_start": 12.5, "za_start": 33.25, "refdm": 56.77}
    with open(src, "wb") as f:
        f.write(sigproc._header_bytes(hdr))
        f.write(np.zeros((3, nchans), np.uint8).tobytes())
    return sigproc.FilReader(src).header, hdr


def samples(nbits, nsamps, nchans, seed):
    rng = np.random.default_rng(seed)
    if nbits == 32:
        return rng.standard_normal((nsamps, nchans)).astype(np.float32)
    return rng.integers(0, 1 << nbits, size=(nsamps, nchans)).astype(np.uint16 if nbits == 16 else np.uint8)


@pytest.mark.parametrize("nbits", [1, 2, 4, 8, 16, 32])
def test_write_block_round_trip(tmp_path, nbits):
    nchans = 24
    rhdr, written = source_header(tmp_path, nchans)
    assert rhdr["nsamples"] == 3 and "hdrlen" in rhdr and "fbottom" in rhdr
    x = samples(nbits, 157, nchans, seed=nbits)
    out = str(tmp_path / "out.fil")
    with sigproc.FilWriter(out, rhdr, nbits=nbits) as w:
        for a, b in ((0, 50), (50, 51), (51, 157)):
            w.write_block(x[a:b])
        assert w.nsamples == 157
    fil = sigproc.FilReader(out)
    assert fil.header["nsamples"] == 157 and fil.header["nbits"] == nbits and fil.header["nifs"] == 1
    for k, v in written.items():
        if k != "nbits":
            assert fil.header[k] == v, k
    np.testing.assert_array_equal(fil.readBlock(0, 157), x.T)


def test_header_order_is_fixed(tmp_path):
    """The same keys in another dict order give the same file."""
    rhdr, _ = source_header(tmp_path, 16)
    names = []
    for i, hdr in enumerate((rhdr, dict(reversed(list(rhdr.items()))))):
        names.append(str(tmp_path / f"o{i}.fil"))
        with sigproc.FilWriter(names[-1], hdr) as w:
            w.write_rows(np.arange(32, dtype=np.uint8).reshape(2, 16))
    assert open(names[0], "rb").read() == open(names[1], "rb").read()


def test_header_validation(tmp_path):
    rhdr, _ = source_header(tmp_path, 20)
    out = str(tmp_path / "bad.fil")
    with pytest.raises(ValueError, match="unknown"):
        sigproc.FilWriter(out, dict(rhdr, observer="nobody"))
    assert not (tmp_path / "bad.fil").exists()         # rejected before the file is created
    with pytest.raises(ValueError, match="lacks"):
        sigproc.FilWriter(out, {k: v for k, v in rhdr.items() if k != "foff"})


def test_partial_byte_and_close(tmp_path):
    rhdr, _ = source_header(tmp_path, 20)
    out = str(tmp_path / "o.fil")
    with pytest.raises(ValueError, match="whole number of bytes"):
        sigproc.FilWriter(out, rhdr, nbits=1)          # 20 bits per spectrum
    with pytest.raises(ValueError, match="not supported"):
        sigproc.FilWriter(out, rhdr, nbits=3)
    w = sigproc.FilWriter(out, rhdr, nbits=2)
    w.write_block(np.ones((4, 20), np.uint8))
    with pytest.raises(ValueError):
        w.write_block(np.ones((4, 19), np.uint8))      # wrong channel count
    with pytest.raises(ValueError):
        w.write_rows(np.ones((4, 6), np.uint8))        # rows are 5 bytes
    w.close()
    w.close()
    assert sigproc.FilReader(out).header["nsamples"] == 4
    with pytest.raises(ValueError, match="closed"):
        w.write_block(np.ones((4, 20), np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("nbits", [1, 2, 4, 8, 32])
def test_write_block_device_equals_host_packing(gpu, tmp_path, nbits):
    """write_block_device of a float64 block = write_block of the numpy-quantised block, byte
    for byte, with a last block of another length."""
    import torch
    nchans, lens = 72, (300, 300, 131)
    rhdr, _ = source_header(tmp_path, nchans)
    rng = np.random.default_rng(100 + nbits)
    top = (1 << min(nbits, 8)) - 1
    x = rng.standard_normal((nchans, sum(lens)))
    scale = rng.uniform(0.5, 2.0, nchans) * (top + 1) / 4
    offset = np.full(nchans, top / 2)
    dev, host = str(tmp_path / "dev.fil"), str(tmp_path / "host.fil")
    with sigproc.FilWriter(dev, rhdr, nbits=nbits) as wd, sigproc.FilWriter(host, rhdr, nbits=nbits) as wh:
        a = 0
        for n in lens:
            blk = x[:, a:a + n]
            a += n
            v = blk * scale[:, None] + offset[:, None]
            if nbits == 32:
                wd.write_block_device(torch.from_numpy(np.ascontiguousarray(blk)).to(gpu), scale, offset)
                wh.write_block(np.ascontiguousarray(v.astype(np.float32).T))
            else:
                # (a view with the plane's row stride: write_block_device takes any row stride)
                wd.write_block_device(torch.from_numpy(x).to(gpu)[:, a - n:a], scale, offset)
                wh.write_block(np.clip(np.rint(v), 0, top).astype(np.uint8).T)
        assert wd.nsamples == wh.nsamples == sum(lens)
    assert open(dev, "rb").read() == open(host, "rb").read()
