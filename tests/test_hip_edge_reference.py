r"""The device against the REFERENCE on the tree edge-case families, without the oracle in between.  Every recorded case of
edge_reference_cases.py (at most 24 000 rows) goes through the public bblean_amd.BitBirch - the default engine, the default
kernel switches - with the fit calls the generator gave the reference, and must equal what the reference's own BitBirch
recorded in tests/golden/edges.npz: the cluster count after every fit call, the assignments, the unsorted member order and
the centroids.  For the split cases the whole tree is compared as well: the pre-order walk of a saved image
(tree_image_format.Image.walk, as in test_hip_tree_splits.py) - per node depth, leaf flag, length and chain position, per
row n_samples, centroid and linear sum, the tracking rows of the internal nodes included.

Only the fixture is read here, never the reference.  The kernel switches are read once per process and the switch matrix
is held against the oracle by test_hip_tree_thresholds.py, test_hip_tree_splits.py and test_hip_tree_storage.py; the oracle
is held against the same fixture by test_edge_reference.py.  The 11 recorded cases of more than 24 000 rows (the mixed
ladder cases, 24 727 rows, and the tier cases, 24 300) run on the oracle only.

Measured on one MI355X: 211 cases in 24 s, the slowest (a prefixed split tail with its image walk) 0.8 s."""
from __future__ import annotations

import tempfile

import pytest

import edge_reference_cases as E
import tree_image_format as IMG

pytestmark = pytest.mark.gpu

CASES = [cid for cid in E.RECORDED if cid in E.fixture() and int(E.fixture()[cid]["numbers"][0]) <= E.GPU_MAX_ROWS]


def image_walk(tree):
    with tempfile.TemporaryFile() as f:
        tree._engine.save_image(f)
        f.seek(0)
        return IMG.Image(bytearray(f.read())).walk()


@pytest.mark.parametrize("cid", CASES)
def test_device_equals_reference(cid):
    from bblean_amd import BitBirch

    c, ops = E.build(cid)
    assert E.input_digest(ops) == bytes(E.fixture()[cid]["input_sha"]).hex(), "the case's rows are not the ones the fixture was made from"
    tree, obs = E.public_observables(BitBirch, c, ops)
    try:
        if cid.startswith("split"):
            walk = image_walk(tree)
            IMG.check_walk(walk, f"{cid}: image")
            obs.update(E.walk_observables(walk), ls=E.sparse_rows(IMG.walk_leaves(walk)["ls"]))
    finally:
        tree._engine.close()
    bad = E.against_fixture(cid, obs)
    assert not bad, f"{cid}: the device differs from the reference in " + "; ".join(bad)
