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


# the order header keys are written in (strings, then integers, then doubles); a key the
# header does not hold is skipped
_HEADER_ORDER = ("source_name", "rawdatafile",
                 "machine_id", "telescope_id", "data_type", "barycentric", "pulsarcentric", "nchans", "nbits", "nifs",
                 "nbeams", "ibeam",
                 "fch1", "foff", "tstart", "tsamp", "az_start", "za_start", "src_raj", "src_dej", "refdm", "period")
# what read_header derives from the file rather than reads from it
_DERIVED_KEYS = ("nsamples", "bandwidth", "ftop", "fbottom", "fcenter", "hdrlen")


def _header_bytes(hdr):
    """The SIGPROC header of the keys in ``hdr``, written in ``_HEADER_ORDER``."""
    def s(x):
        b = x.encode()
        return struct.pack("<i", len(b)) + b

    unknown = sorted(set(hdr) - set(_HEADER_ORDER))
    if unknown:
        raise ValueError(f"unknown SIGPROC header key(s) {unknown}")
    out = [s("HEADER_START")]
    for k in _HEADER_ORDER:
        if k not in hdr:
            continue
        if k in _STR_KEYS:
            out += [s(k), s(str(hdr[k]))]
        elif k in _INT_KEYS:
            out += [s(k), struct.pack("<i", int(hdr[k]))]
        else:
            out += [s(k), struct.pack("<d", float(hdr[k]))]
    out.append(s("HEADER_END"))
    return b"".join(out)


def write_filterbank(fname, data_tc, fch1, foff, tsamp, tstart=60000.0, source_name="synthetic", nbits=None):
    """Write a time-major (nsamps, nchans) array as a SIGPROC filterbank file.

    ``nbits`` 1, 2 or 4 packs an integer array (values below ``2**nbits``) in the bit order of
    the module docstring; otherwise the array's bytes are written as they are."""
    data_tc = np.ascontiguousarray(data_tc)
    nchans = data_tc.shape[1]
    if nbits in _PACKED:
        data_tc = _pack(data_tc, nbits)
    nbits = nbits or {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16, np.dtype(np.float32): 32}[data_tc.dtype]
    hdr = {"source_name": source_name, "machine_id": 0, "telescope_id": 0, "data_type": 1, "nchans": nchans,
           "nbits": nbits, "nifs": 1, "fch1": fch1, "foff": foff, "tstart": tstart, "tsamp": tsamp}
    with open(fname, "wb") as f:
        f.write(_header_bytes(hdr))
        f.write(data_tc.tobytes())


class FilWriter:
    """Streaming SIGPROC writer (a context manager): the header goes out at open, sample rows
    are appended block by block, so a file never has to exist whole in memory.

    ``header``: a dict as in :attr:`FilReader.header`.  The keys read_header derives
    (``nsamples, bandwidth, ftop, fbottom, fcenter, hdrlen``) are dropped, ``nifs`` is
    written as 1 (blocks hold one IF) and ``nbits`` (when given) replaces the header's value;
    every other key must be one of the module's ``_INT_KEYS`` / ``_DBL_KEYS`` / ``_STR_KEYS``
    (``ValueError`` otherwise) and is written through unchanged, in the fixed order
    ``_HEADER_ORDER``: source_name, rawdatafile; machine_id, telescope_id, data_type,
    barycentric, pulsarcentric, nchans, nbits, nifs, nbeams, ibeam; fch1, foff, tstart, tsamp,
    az_start, za_start, src_raj, src_dej, refdm, period.  ``nchans, fch1, foff, tsamp`` are
    required (FilReader cannot open a file without them).

    ``write_block`` takes host time-major samples, ``write_block_device`` a channel-major
    device block (quantised, transposed and packed on the GPU, pu_quantize_pack_transpose:
    only ``nbits / 8`` bytes per sample cross PCIe), ``write_rows`` rows that are packed
    already.  ``nsamples`` counts the spectra written so far."""

    def __init__(self, fname, header, nbits=None):
        hdr = {k: v for k, v in dict(header).items() if k not in _DERIVED_KEYS}
        missing = [k for k in ("nchans", "fch1", "foff", "tsamp") if k not in hdr]
        if missing:
            raise ValueError(f"FilWriter: header lacks {missing}")
        hdr["nifs"] = 1
        hdr["nbits"] = int(nbits if nbits is not None else hdr.get("nbits", 8))
        self.nbits, self.nchans = hdr["nbits"], int(hdr["nchans"])
        if self.nbits not in _DTYPES and self.nbits not in _PACKED:
            raise ValueError(f"FilWriter: nbits={self.nbits} not supported (1, 2, 4, 8, 16, 32)")
        if self.nchans < 1 or self.nchans * self.nbits % 8:
            raise ValueError(f"FilWriter: nchans={self.nchans} x nbits={self.nbits} is not a whole number of bytes "
                             "per spectrum")
        head = _header_bytes(hdr)  # (an unknown key raises before the file is created)
        self.filename = fname
        self.header = hdr
        self.row_bytes = self.nchans * self.nbits // 8
        self.nsamples = 0
        self._f = open(fname, "wb")
        self._f.write(head)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        """Flush and close the file; further calls do nothing."""
        if self._f is not None:
            self._f.close()
            self._f = None

    def write_rows(self, rows):
        """Append packed host rows: a 2-D array whose rows are ``row_bytes`` bytes each."""
        if self._f is None:
            raise ValueError("FilWriter: the file is closed")
        rows = np.ascontiguousarray(rows)
        if rows.ndim != 2 or rows.shape[1] * rows.itemsize != self.row_bytes:
            raise ValueError(f"FilWriter: rows of {self.row_bytes} bytes expected, got shape {rows.shape} of "
                             f"{rows.dtype}")
        self._f.write(rows.data)
        self.nsamples += rows.shape[0]

    def write_block(self, data_tc):
        """Append a host time-major (nsamps, nchans) block: an integer array below ``2**nbits``
        for 1-, 2- and 4-bit output (packed by ``_pack``), otherwise an array of the file's
        dtype (uint8, uint16 or float32), written as it is."""
        data_tc = np.asarray(data_tc)
        if data_tc.ndim != 2 or data_tc.shape[1] != self.nchans:
            raise ValueError(f"FilWriter: a (nsamps, {self.nchans}) block expected, got shape {data_tc.shape}")
        if self.nbits in _PACKED:
            rows = _pack(np.ascontiguousarray(data_tc), self.nbits)
        elif data_tc.dtype != np.dtype(_DTYPES[self.nbits]):
            raise ValueError(f"FilWriter: {self.nbits}-bit output takes {np.dtype(_DTYPES[self.nbits])} blocks, got "
                             f"{data_tc.dtype}")
        else:
            rows = data_tc
        self.write_rows(rows)

    def write_block_device(self, x, scale=None, offset=None):
        """Append a channel-major (nchans, nsamps) device block through
        :func:`quantize_pack_device` (``nbits`` 1, 2, 4, 8 or 32); synchronises on the copy."""
        if self.nbits not in (1, 2, 4, 8, 32):
            raise ValueError(f"FilWriter: write_block_device writes 1, 2, 4, 8 or 32 bits, not {self.nbits}")
        if x.dim() != 2 or x.shape[0] != self.nchans:
            raise ValueError(f"FilWriter: a ({self.nchans}, nsamps) block expected, got shape {tuple(x.shape)}")
        self.write_rows(quantize_pack_device(x, self.nbits, scale, offset).cpu().numpy())


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

    def upload_block(self, start, nsamps, device=None, stream=None):
        """The time-major rows of ``_block_tc`` as stored (packed bytes still packed) on the device: a
        pageable copy from the memory map on ``stream`` (default: the current one)."""
        from . import _hip
        t = _hip.require_gpu()
        tc = np.ascontiguousarray(self._block_tc(start, nsamps))
        with t.cuda.stream(stream):  # (no stream: nothing to enter)
            return t.from_numpy(tc).to(device or t.device("cuda", t.cuda.current_device()))

    def read_block_device(self, start, nsamps, device=None):
        """(nchans, nsamps) device tensor: time-major bytes uploaded (packed ones still
        packed), transposed by pu_transpose / unpacked by pu_unpack_transpose."""
        return self.device_block(self.upload_block(start, nsamps, device))

    def device_block(self, src):
        """Channel-major (nchans, nsamps) device tensor of an uploaded time-major block (the
        rows of ``upload_block``): ``uint8`` unpacked by pu_unpack_transpose for 1/2/4-bit
        files, the file's dtype transposed by pu_transpose otherwise."""
        if self.packed:
            return unpack_transpose_device(src, self.nbits, self.header["nchans"])
        return transpose_device(src)


def transpose_device(src):
    """(rows, cols) -> (cols, rows) contiguous, HIP tiled transpose (1/2/4/8-byte elements).
    ``src`` may have any row stride; its columns must be adjacent (unit column stride)."""
    from . import _hip
    t = _hip.require_gpu()
    if src.dim() != 2 or not src.is_cuda or (src.shape[1] > 1 and src.stride(1) != 1):
        raise ValueError("transpose_device: a 2-D CUDA tensor with unit column stride")
    rows, cols = src.shape
    out = t.empty((cols, rows), dtype=src.dtype, device=src.device)
    _hip.check(_hip.lib().pu_transpose(_hip.ptr(src), src.element_size(), rows, cols, _hip.row_stride(src),
                                       _hip.ptr(out), rows, _hip.stream_ptr()), "pu_transpose")
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
    _hip.check(_hip.lib().pu_unpack_transpose(_hip.ptr(src), nbits, nsamps, nchans, _hip.row_stride(src),
                                              _hip.ptr(out), nsamps, _hip.stream_ptr()), "pu_unpack_transpose")
    return out


def quantize_pack_device(x, nbits, scale=None, offset=None):
    """Channel-major (nchans, nsamps) device block -> SIGPROC sample rows on the device: the
    inverse of :func:`unpack_transpose_device` (pu_quantize_pack_transpose).

    ``v = x[c, t] * scale[c] + offset[c]`` in float64 (``v = x`` when both are None); for
    ``nbits`` 1, 2, 4, 8 a NaN becomes ``offset[c]`` (0 without an offset), ``q = clip(rint(v),
    0, 2**nbits - 1)`` is packed in the bit order of the module docstring and the result is a
    contiguous ``(nsamps, nchans * nbits / 8)`` uint8 tensor; ``nbits == 32`` returns
    ``(nsamps, nchans)`` float32 of ``v`` (no clamp, NaN kept).  ``x``: uint8, float32 or
    float64 with unit column stride and any row stride; ``scale``, ``offset``: numpy or device
    float64 ``[nchans]``."""
    from . import _hip
    t = _hip.require_gpu()
    nbits = int(nbits)
    code = _hip.dtype_code(x.dtype) if isinstance(x, t.Tensor) else None
    if (code not in (_hip.PU_U8, _hip.PU_F32, _hip.PU_F64) or x.dim() != 2 or not x.is_cuda
            or (x.shape[1] > 1 and x.stride(1) != 1)):
        raise ValueError("quantize_pack_device: a 2-D uint8 / float32 / float64 CUDA tensor with unit column stride")
    nchans, nsamps = x.shape

    def vec(a, name):
        if a is None:
            return None
        if not isinstance(a, t.Tensor):
            a = t.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        a = a.to(x.device)
        if a.dtype != t.float64 or tuple(a.shape) != (nchans,):
            raise ValueError(f"quantize_pack_device: {name} must be float64 of shape ({nchans},), got {a.dtype} "
                             f"{tuple(a.shape)}")
        return a.contiguous()

    scale, offset = vec(scale, "scale"), vec(offset, "offset")
    if nbits == 32:
        out = t.empty((nsamps, nchans), dtype=t.float32, device=x.device)
    else:
        # (a width the library does not write, or a partial byte per spectrum, is its error to raise)
        out = t.empty((nsamps, nchans * nbits // 8), dtype=t.uint8, device=x.device)
    valid = nbits == 32 or (nbits in _PACKED + (8,) and nchans * nbits % 8 == 0)
    if valid and (scale is None) == (offset is None) and x.numel() == 0:
        return out  # (an empty tensor has no pointer to pass)
    _hip.check(_hip.lib().pu_quantize_pack_transpose(_hip.ptr(x), code, nchans, nsamps, _hip.row_stride(x),
                                                     _hip.ptr(scale), _hip.ptr(offset), nbits, _hip.ptr(out),
                                                     out.shape[1] * out.element_size(), _hip.stream_ptr()),
               "pu_quantize_pack_transpose")
    return out
