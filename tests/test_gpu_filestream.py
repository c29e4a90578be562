"""filestream.ChunkStream on 8-bit, 2-bit packed, 16-bit and float32 files: the chunks it yields
and every block against FilReader.readBlock, with and without the loader thread, and that
leaving the ``with`` early (``break``, an exception in the loop body) leaves no thread behind."""
import threading

import numpy as np
import pytest

from pulsarutils import sigproc
from pulsarutils.filestream import ChunkStream, tiled_chunks

pytestmark = pytest.mark.gpu

NCH, NS = 64, 5000
HDR = dict(fch1=1500.0, foff=-300.0 / NCH, tsamp=64e-6)
KINDS = {"u8": (np.uint8, 256, None), "2bit": (np.uint8, 4, 2), "u16": (np.uint16, 60000, None),
         "f32": (np.float32, 1000, None)}


@pytest.fixture(scope="module")
def files(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("filestream")
    out = {}
    for seed, (kind, (dtype, top, nbits)) in enumerate(KINDS.items()):
        x = np.random.default_rng(300 + seed).integers(0, top, size=(NS, NCH)).astype(dtype)
        out[kind] = str(d / f"{kind}.fil")
        sigproc.write_filterbank(out[kind], x, nbits=nbits, **HDR)
    return out


@pytest.mark.parametrize("chunksize", [1024, 2048])     # 2048: the 904-sample tail is merged
@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("kind", list(KINDS))
def test_blocks_equal_read_block(gpu, files, kind, prefetch, chunksize):
    import torch
    fil = sigproc.FilReader(files[kind])
    chunks = tiled_chunks(0, NS, chunksize)
    want_dtype = {"u8": torch.uint8, "2bit": torch.uint8, "u16": torch.float64, "f32": torch.float32}[kind]
    seen = []
    with ChunkStream(fil, chunks, gpu, prefetch=prefetch) as blocks:
        for istart, size, block in blocks:
            seen.append((istart, size))
            assert block.dtype == want_dtype and block.device == gpu and block.is_contiguous()
            assert tuple(block.shape) == (NCH, size)
            np.testing.assert_array_equal(block.cpu().numpy(), fil.readBlock(istart, size))
    assert seen == chunks and len(chunks) == (5 if chunksize == 1024 else 2)


def test_break_leaves_no_loader_thread(gpu, files):
    fil = sigproc.FilReader(files["u8"])
    before = set(threading.enumerate())
    with ChunkStream(fil, tiled_chunks(0, NS, 1024), gpu, prefetch=True) as blocks:
        assert set(threading.enumerate()) - before, "the loader thread runs inside the with"
        for istart, size, block in blocks:
            break
    assert set(threading.enumerate()) == before
    assert blocks._pending is None                      # the chunk loaded ahead is dropped


def test_exception_leaves_no_loader_thread(gpu, files):
    fil = sigproc.FilReader(files["u8"])
    before = set(threading.enumerate())
    with pytest.raises(RuntimeError, match="chunk 0 failed") as caught:
        with ChunkStream(fil, tiled_chunks(0, NS, 1024), gpu, prefetch=True) as blocks:
            for istart, size, block in blocks:
                raise RuntimeError("chunk 0 failed")
    # (``caught`` holds the traceback, and so the loop's frame, alive here)
    assert caught.value is not None and set(threading.enumerate()) == before
    assert blocks._pending is None
