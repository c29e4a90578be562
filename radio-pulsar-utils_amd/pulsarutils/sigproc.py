"""SIGPROC filterbank I/O (replaces ``sigpyproc.Readers.FilReader`` for the hot path).

The reference reads files through sigpyproc (``stats.py:36-45``, ``clean.py:284-327``) and
uses these header keys: ``nsamples, tsamp, fbottom, ftop, bandwidth, nchans, foff,
tstart`` (``clean.py:286-294``) and ``readBlock(start, nsamps, as_filterbankBlock=False)``
-> ``(nchans, nsamps)`` (``clean.py:327``, ``stats.py:45``).  sigpyproc is not available in
this image; derived keys follow sigpyproc's Header conventions (parity unpinned by the
reference's tests, which never read a file):

    bandwidth = |foff| * nchans
    ftop      = fch1 - 0.5 * foff
    fbottom   = ftop + foff * nchans        (lower band edge when foff < 0)
    nsamples  = data bytes / (nchans * nifs * nbits / 8)

Samples are memory-mapped (never loaded whole).  The on-disk layout is time-major
(one spectrum per sample); :meth:`FilReader.readBlock` returns channel-major
``(nchans, nsamps)`` like sigpyproc, :meth:`FilReader.read_block_device` transposes on
the GPU (``pu_transpose``) so large blocks never go through a host transpose.

Sample widths: ``nbits`` 8 (uint8), 16 (uint16), 32 (float32) and the packed widths 1, 2
and 4.  A packed spectrum holds channel ``c`` in bits ``[c * nbits, (c + 1) * nbits)``
counted from the least-significant bit of its first byte (the sigproc / sigpyproc order:
the first channel sits in the low bits), so ``nchans * nbits`` must be a whole number of
bytes.  Packed data is read as unsigned values into ``uint8``: ``readBlock`` unpacks on
the host (API parity, not a hot path), ``read_block_device`` uploads the packed bytes and
unpacks + transposes them on the GPU (``pu_unpack_transpose``), after which the block is an
ordinary 8-bit one.  MSB-first and signed packings are not supported.
"""
import os
import struct

import numpy as np

_INT_KEYS = {"telescope_id", "machine_id", "data_type", "barycentric", "pulsarcentric", "nbits", "nsamples",
             "nchans", "nifs", "nbeams", "ibeam"}
_DBL_KEYS = {"az_start", "za_start", "src_raj", "src_dej", "tstart", "tsamp", "fch1", "foff", "refdm",
             "period"}
_STR_KEYS = {"source_name", "rawdatafile"}
_DTYPES = {8: np.uint8, 16: np.uint16, 32: np.float32}
_PACKED = (1, 2, 4)


def _rd_str(f):
    (n,) = struct.unpack("<i", f.read(4))
    if not 0 < n < 4096:
        raise ValueError("not a SIGPROC header (bad string length)")
    return f.read(n).decode("ascii", errors="replace")


def read_header(fname):
    """Parse a SIGPROC header; returns (dict, header_bytes)."""
    hdr = {}
    with open(fname, "rb") as f:
        if _rd_str(f) != "HEADER_START":
            raise ValueError(f"{fname}: missing HEADER_START")
        while True:
            key = _rd_str(f)
            if key == "HEADER_END":
                break
            if key in _INT_KEYS:
                (hdr[key],) = struct.unpack("<i", f.read(4))
            elif key in _DBL_KEYS:
                (hdr[key],) = struct.unpack("<d", f.read(8))
            elif key in _STR_KEYS:
                hdr[key] = _rd_str(f)
            else:
                raise ValueError(f"{fname}: unknown SIGPROC header key {key!r}")
        hdr_len = f.tell()
    nbits = hdr.get("nbits", 8)
    nchans = hdr["nchans"]
    nifs = hdr.get("nifs", 1)
    if nbits < 1 or nchans * nbits % 8:
        raise ValueError(f"{fname}: nchans={nchans} x nbits={nbits} is not a whole number of bytes per spectrum")
    data_bytes = os.path.getsize(fname) - hdr_len
    hdr.setdefault("nifs", 1)
    hdr["nsamples"] = data_bytes // (nchans * nifs * nbits // 8)
    foff = hdr["foff"]
    hdr["bandwidth"] = abs(foff) * nchans
    hdr["ftop"] = hdr["fch1"] - 0.5 * foff
    hdr["fbottom"] = hdr["ftop"] + foff * nchans
    hdr["fcenter"] = hdr["ftop"] + 0.5 * foff * nchans
    hdr["hdrlen"] = hdr_len
    return hdr, hdr_len


def _pack(data_tc, nbits):
    """(nsamps, nchans) unsigned values below 2**nbits -> (nsamps, nchans * nbits / 8) packed bytes."""
    nsamps, nchans = data_tc.shape
    if nchans * nbits % 8:
        raise ValueError(f"nchans={nchans} x nbits={nbits} is not a whole number of bytes per spectrum")
    if data_tc.dtype.kind not in "ui":
        raise ValueError(f"packing to {nbits} bits needs an integer array, got {data_tc.dtype}")
    if data_tc.size and (data_tc.min() < 0 or data_tc.max() >= 1 << nbits):
        raise ValueError(f"values outside [0, {(1 << nbits) - 1}] do not fit in {nbits} bits")
    shifts = np.arange(8 // nbits, dtype=np.uint8) * nbits
    return np.bitwise_or.reduce(data_tc.astype(np.uint8).reshape(nsamps, nchans * nbits // 8, 8 // nbits) << shifts,
                                axis=2)


def _unpack(packed, nbits):
    """(nsamps, bytes) packed rows -> (nsamps, bytes * 8 / nbits) uint8 values (host, numpy)."""
    shifts = np.arange(8 // nbits, dtype=np.uint8) * nbits
    return ((packed[:, :, None] >> shifts) & np.uint8((1 << nbits) - 1)).reshape(packed.shape[0],
                                                                                        packed.shape[1] * (8 // nbits))


def write_filterbank(fname, data_tc, fch1, foff, tsamp, tstart=60000.0, source_name="synthetic", nbits=None):
    """Write a time-major (nsamps, nchans) array as a SIGPROC filterbank file.

    ``nbits`` 1, 2 or 4 packs an integer array (values below ``2**nbits``) in the bit order of
    the module docstring; otherwise the array's bytes are written as they are."""
    data_tc = np.ascontiguousarray(data_tc)
    nchans = data_tc.shape[1]
    if nbits in _PACKED:
        data_tc = _pack(data_tc, nbits)
    nbits = nbits or {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16, np.dtype(np.float32): 32}[data_tc.dtype]

    def s(x):
        b = x.encode()
        return struct.pack("<i", len(b)) + b

    out = [s("HEADER_START"), s("source_name"), s(source_name)]
    for k, v in (("machine_id", 0), ("telescope_id", 0), ("data_type", 1), ("nchans", nchans),
                 ("nbits", nbits), ("nifs", 1)):
        out += [s(k), struct.pack("<i", v)]
    for k, v in (("fch1", fch1), ("foff", foff), ("tstart", tstart), ("tsamp", tsamp)):
        out += [s(k), struct.pack("<d", v)]
    out.append(s("HEADER_END"))
    with open(fname, "wb") as f:
        f.write(b"".join(out))
        f.write(data_tc.tobytes())


class FilReader:
    """Memory-mapped SIGPROC reader with sigpyproc's ``header`` / ``readBlock`` surface."""

    def __init__(self, fname):
        self.filename = fname
        self.header, self._hdr_len = read_header(fname)
        nbits = self.header.get("nbits", 8)
        if nbits not in _DTYPES and nbits not in _PACKED:
            raise ValueError(f"{fname}: nbits={nbits} not supported (1, 2, 4, 8, 16, 32)")
        self.nbits = nbits
        self.packed = nbits in _PACKED
        self.dtype = np.dtype(np.uint8 if self.packed else _DTYPES[nbits])
        # elements of the memory map per spectrum / per IF: packed bytes for 1/2/4-bit data
        per_if = self.header["nchans"] * nbits // 8 if self.packed else self.header["nchans"]
        self._row = per_if
        self._mm = np.memmap(fname, dtype=self.dtype, mode="r", offset=self._hdr_len,
                             shape=(self.header["nsamples"], per_if * self.header["nifs"]))

    def _block_tc(self, start, nsamps):
        """Time-major rows of the first IF as stored: samples, or packed bytes (1/2/4-bit)."""
        start = int(start)
        nsamps = int(min(nsamps, self.header["nsamples"] - start))
        if start < 0 or nsamps < 0:
            raise ValueError("block outside the file")
        return self._mm[start:start + nsamps, :self._row]

    def readBlock(self, start, nsamps, as_filterbankBlock=False):  # noqa: N802 (sigpyproc name)
        """(nchans, nsamps) array in file channel order (host transpose; packed files are
        unpacked to uint8 on the host first)."""
        tc = self._block_tc(start, nsamps)
        if self.packed:
            tc = _unpack(tc, self.nbits)
        return np.ascontiguousarray(tc.T)

    def read_block_device(self, start, nsamps, device=None):
        """(nchans, nsamps) device tensor: time-major bytes uploaded (packed ones still
        packed), transposed by pu_transpose / unpacked by pu_unpack_transpose."""
        from . import _hip
        t = _hip.require_gpu()
        tc = np.ascontiguousarray(self._block_tc(start, nsamps))
        src = t.from_numpy(tc).to(device or t.device("cuda", t.cuda.current_device()))
        return self.device_block(src)

    def device_block(self, src):
        """Channel-major (nchans, nsamps) device tensor of an uploaded time-major block (the
        rows of ``_block_tc``): ``uint8`` unpacked by pu_unpack_transpose for 1/2/4-bit
        files, the file's dtype transposed by pu_transpose otherwise."""
        if self.packed:
            return unpack_transpose_device(src, self.nbits, self.header["nchans"])
        return transpose_device(src)


def transpose_device(src):
    """(rows, cols) -> (cols, rows) contiguous, HIP tiled transpose (1/2/4/8-byte elements)."""
    from . import _hip
    t = _hip.require_gpu()
    rows, cols = src.shape
    out = t.empty((cols, rows), dtype=src.dtype, device=src.device)
    _hip.check(_hip.lib().pu_transpose(_hip.ptr(src), src.element_size(), rows, cols, src.stride(0), _hip.ptr(out),
                                       rows, _hip.stream_ptr()), "pu_transpose")
    return out


def unpack_transpose_device(src, nbits, nchans):
    """(nsamps, >= nchans * nbits / 8) packed uint8 rows -> (nchans, nsamps) uint8 contiguous:
    HIP unpack + transpose of 1/2/4-bit samples (pu_unpack_transpose; bit order in the module
    docstring).  ``src`` may start at any byte and have any row stride."""
    from . import _hip
    t = _hip.require_gpu()
    nbits, nchans = int(nbits), int(nchans)
    if src.dim() != 2 or src.dtype != t.uint8 or not src.is_cuda or (src.shape[1] > 1 and src.stride(1) != 1):
        raise ValueError("unpack_transpose_device: a 2-D uint8 CUDA tensor with unit column stride")
    nsamps = src.shape[0]
    # (a width the library does not unpack, or a partial byte per spectrum, is its error to raise)
    if nchans < 0 or (nbits in _PACKED and src.shape[1] < nchans * nbits // 8):
        raise ValueError(f"unpack_transpose_device: rows of {src.shape[1]} bytes do not hold {nchans} "
                         f"{nbits}-bit channels")
    out = t.empty((nchans, nsamps), dtype=t.uint8, device=src.device)
    if nbits in _PACKED and out.numel() == 0:
        return out  # (an empty tensor has no pointer to pass)
    # a single row's stride is arbitrary in torch: any value >= the row's bytes will do
    ld_src = src.stride(0) if nsamps > 1 else max(src.stride(0), src.shape[1])
    _hip.check(_hip.lib().pu_unpack_transpose(_hip.ptr(src), nbits, nsamps, nchans, ld_src, _hip.ptr(out),
                                              nsamps, _hip.stream_ptr()), "pu_unpack_transpose")
    return out
