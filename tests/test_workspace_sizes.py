"""Every ``pu_*_workspace_bytes`` function returns the sizes recorded in
tests/golden/workspace_sizes.json (no GPU needed).  The table was taken from the library
before the workspace layouts moved to ``pu::Carver``: zero and negative sizes, one row and a
few, lengths below, at and just above the segment and tile sizes (8192, 16384; 2^13 and 2^14
for ``nfft``), and for every function that detects overflow an argument set that overflows.
``pu_plan_workspace_bytes`` takes a plan, which needs a device, and is not in the table."""
import json
import os

import pytest

from conftest import REPO

with open(os.path.join(REPO, "tests", "golden", "workspace_sizes.json")) as _f:
    GOLDEN = json.load(_f)


def test_table_covers_every_size_function():
    from pulsarutils import _hip
    names = {n for n in _hip.SIGNATURES if n.endswith("_workspace_bytes")} - {"pu_plan_workspace_bytes"}
    assert names == set(GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_workspace_sizes(name):
    from pulsarutils import _hip
    fn = getattr(_hip.lib(), name)
    got = [[args, int(fn(*args))] for args, _ in GOLDEN[name]]
    assert got == GOLDEN[name]
