"""1-, 2- and 4-bit SIGPROC files on the host: the bit order (pinned by literal bytes),
write_filterbank -> FilReader.readBlock round trips, and the argument checks of the writer,
the reader and pu_unpack_transpose (made before any HIP call: no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest

from pulsarutils import sigproc

# one spectrum of 8 channels per width and its packed bytes: channel c sits in bits
# [c * nbits, (c + 1) * nbits) counted from the least-significant bit of byte 0
# (for 1 bit the asymmetric pattern 1,0,0,0,0,0,1,1 is 0xC1 by that rule - bits 0, 6 and 7 -
# and 0xC3 is 1,1,0,0,0,0,1,1; both are pinned, 0xC1 being the one that tells the bit
# order: most-significant-first would give 0x83)
LITERAL = [
    (1, [1, 0, 0, 0, 0, 0, 1, 1], bytes([0xC1])),
    (1, [1, 1, 0, 0, 0, 0, 1, 1], bytes([0xC3])),
    (2, [0, 1, 2, 3, 3, 2, 1, 0], bytes([0xE4, 0x1B])),
    (4, [1, 10, 15, 0, 7, 8, 0, 5], bytes([0xA1, 0x0F, 0x87, 0x50])),
]
HDR = dict(fch1=1500.0, foff=-1.0, tsamp=1e-3)


@pytest.mark.parametrize("nbits,values,packed", LITERAL)
def test_writer_bit_order_literal(tmp_path, nbits, values, packed):
    fname = str(tmp_path / "lit.fil")
    sigproc.write_filterbank(fname, np.array([values], np.uint8), nbits=nbits, **HDR)
    hdr, hdr_len = sigproc.read_header(fname)
    assert hdr["nbits"] == nbits and hdr["nchans"] == 8 and hdr["nsamples"] == 1
    assert open(fname, "rb").read()[hdr_len:] == packed


@pytest.mark.parametrize("nbits,values,packed", LITERAL)
def test_reader_bit_order_literal(tmp_path, nbits, values, packed):
    """The file's data bytes are the literal ones (the header alone comes from the writer,
    by way of an empty file)."""
    fname = str(tmp_path / "lit.fil")
    sigproc.write_filterbank(fname, np.zeros((0, 8), np.uint8), nbits=nbits, **HDR)
    with open(fname, "ab") as f:
        f.write(packed * 3)
    fil = sigproc.FilReader(fname)
    assert fil.nbits == nbits and fil.dtype == np.uint8 and fil.header["nsamples"] == 3
    blk = fil.readBlock(0, 3)
    assert blk.dtype == np.uint8 and blk.shape == (8, 3) and blk.flags.c_contiguous
    np.testing.assert_array_equal(blk, np.repeat(np.array(values, np.uint8)[:, None], 3, axis=1))


@pytest.mark.parametrize("nbits,nsamps,nchans", [(1, 37, 8), (1, 50, 40), (2, 33, 20), (2, 101, 64), (4, 29, 6),
                                                 (4, 64, 130)])
def test_round_trip(tmp_path, nbits, nsamps, nchans):
    """(2, 33, 20) and (1, 50, 40) have rows of 5 bytes, (4, 29, 6) of 3."""
    rng = np.random.default_rng(nbits * 1000 + nchans)
    x = rng.integers(0, 1 << nbits, size=(nsamps, nchans)).astype(np.uint8)
    fname = str(tmp_path / "rt.fil")
    sigproc.write_filterbank(fname, x, nbits=nbits, **HDR)
    hdr, hdr_len = sigproc.read_header(fname)
    assert os.path.getsize(fname) - hdr_len == nsamps * nchans * nbits // 8
    fil = sigproc.FilReader(fname)
    assert fil.header["nsamples"] == nsamps and fil.header["nchans"] == nchans
    np.testing.assert_array_equal(fil.readBlock(0, nsamps), x.T)
    np.testing.assert_array_equal(fil.readBlock(7, 11), x[7:18].T)
    # a block that runs past the end of the file is cut short, as for 8-bit files
    np.testing.assert_array_equal(fil.readBlock(nsamps - 5, 100), x[nsamps - 5:].T)


def test_wider_files_unchanged(tmp_path):
    """nbits=8 given explicitly, or no nbits at all, writes the array's own bytes as before."""
    x = np.arange(48, dtype=np.uint8).reshape(6, 8)
    for kw in ({}, {"nbits": 8}):
        fname = str(tmp_path / "u8.fil")
        sigproc.write_filterbank(fname, x, **HDR, **kw)
        fil = sigproc.FilReader(fname)
        assert fil.nbits == 8 and fil.dtype == np.uint8
        np.testing.assert_array_equal(fil.readBlock(0, 6), x.T)


@pytest.mark.parametrize("nbits", [1, 2, 4])
def test_writer_rejects_values_that_do_not_fit(tmp_path, nbits):
    x = np.zeros((4, 8), np.uint8)
    x[2, 5] = 1 << nbits
    with pytest.raises(ValueError, match="fit"):
        sigproc.write_filterbank(str(tmp_path / "big.fil"), x, nbits=nbits, **HDR)


@pytest.mark.parametrize("nbits,nchans", [(1, 4), (2, 6), (4, 3), (1, 12)])
def test_partial_byte_rows_rejected(tmp_path, nbits, nchans):
    """nchans * nbits not a multiple of 8: ValueError from the writer and from the reader
    (a 1-bit file of 4 channels must not divide by zero)."""
    fname = str(tmp_path / "odd.fil")
    with pytest.raises(ValueError, match="whole number of bytes"):
        sigproc.write_filterbank(fname, np.zeros((4, nchans), np.uint8), nbits=nbits, **HDR)
    # such a file made by other means: the header of an 8-bit file of the same channel
    # count with its nbits value overwritten
    sigproc.write_filterbank(fname, np.zeros((4, nchans), np.uint8), **HDR)
    raw = bytearray(open(fname, "rb").read())
    key = b"\x05\x00\x00\x00nbits"
    at = raw.index(key) + len(key)
    assert raw[at:at + 4] == bytes([8, 0, 0, 0])
    raw[at] = nbits
    open(fname, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="whole number of bytes"):
        sigproc.read_header(fname)
    with pytest.raises(ValueError, match="whole number of bytes"):
        sigproc.FilReader(fname)


def _call(nbits, nsamps, nchans, ld_src, ld_dst, src=0x1000, dst=0x2000):
    """pu_unpack_transpose with pointers that are never dereferenced: every case below is
    turned away by the argument checks, which run before the first HIP call."""
    from pulsarutils import _hip
    lib = _hip.lib()
    rc = lib.pu_unpack_transpose(ctypes.c_void_p(src), nbits, nsamps, nchans, ld_src, ctypes.c_void_p(dst), ld_dst,
                                 None)
    return rc, lib.pu_last_error().decode()


def test_abi_argument_checks():
    # partial bytes per spectrum: 12 channels x 1 bit, 6 x 2, 3 x 4 (12 x 2 bits is 3 whole
    # bytes and valid, like the 5-byte rows of 20 x 2)
    for nbits, nchans in ((1, 12), (2, 6), (4, 3)):
        rc, msg = _call(nbits, 16, nchans, 3, 16)
        assert rc == -1 and "pu_unpack_transpose" in msg
    rc, msg = _call(2, 16, 16, 3, 16)          # rows of 4 bytes, ld_src 3
    assert rc == -1 and "pu_unpack_transpose" in msg
    rc, msg = _call(4, 16, 16, 8, 15)          # ld_dst < nsamps
    assert rc == -1 and "pu_unpack_transpose" in msg
    rc, msg = _call(3, 16, 16, 8, 16)
    assert rc == -4 and "pu_unpack_transpose" in msg
    for nbits in (0, 8, -1):
        assert _call(nbits, 16, 16, 16, 16)[0] == -4
    rc, msg = _call(1, 16, 16, 2, 16, src=None)
    assert rc == -1 and "pu_unpack_transpose" in msg
    rc, msg = _call(1, 16, 16, 2, 16, dst=None)
    assert rc == -1 and "pu_unpack_transpose" in msg
    rc, msg = _call(1, -1, 16, 2, 16)
    assert rc == -1 and "pu_unpack_transpose" in msg
    # more tiles than a grid holds
    rc, msg = _call(1, 1 << 40, 1 << 20, 1 << 17, 1 << 40)
    assert rc == -1 and "grid" in msg


def test_abi_zero_sizes_launch_nothing():
    assert _call(1, 0, 16, 2, 0)[0] == 0
    assert _call(4, 16, 0, 0, 16)[0] == 0
