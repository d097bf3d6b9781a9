"""Every path of the dense diagonalize driver (csrc/eigdec.cpp) and of basis_image (csrc/blockdiag.cpp) against a table recorded
once from the csrc of the commit that tests/golden/dense_paths.json names: tools/record_dense_paths.py holds the rows and the one
way a row is run."""
import importlib.util
import json
import pathlib

import pytest

pytestmark = pytest.mark.gpu


def _tool():
    path = pathlib.Path(__file__).resolve().parents[1] / "tools" / "record_dense_paths.py"
    spec = importlib.util.spec_from_file_location("record_dense_paths", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_dense_path_matches_the_recorded_table(pkg, problems, golden):
    """Forced dense driver (eig_driver = 4).  blockDiagonalize, instance x seed x one flag: the commutative circ256, er7k8
    (n = 456, the largest order here), K17 (eigenspaces of dimension > 1, merged classes: the saved T or, under
    FRESH_IRREDUCIBLE_ELEMENT, a third element), K2, DS, the non-symmetric verdict.  The five basis_image routes of
    test_gpu_outputs.ROUTES on K17, K2, K40, DS: the CRC pins the images bit for bit on two_stage, outer, chunk, both shortcuts
    and FULL_BASIS_IMAGE.  The retry loop made deterministic by d + 1: both extra coupling elements and the fresh third
    element are drawn (5 draws), DIMENSION_MISMATCH with sizes and Q_hat stored.  Six eigen_decomposition calls on one ctx at
    320 eigenspaces (classes on the device, or on the host under COUPLING_ON_HOST; one of the six is inconsistent) and the
    serial branch of the batched entry.  Each row -- status or error code and message, block sizes in order, draw position,
    host waits, CRC32 of Q_hat and of blks, (neig, nclasses) per call -- equals the recorded one."""
    tool = _tool()
    with open(tool.GOLDEN) as f:
        recorded = json.load(f)["rows"]
    rows = tool.rows()
    assert set(recorded) == {row[0] for row in rows} and len(rows) == 101
    for rid, want in recorded.items():  # every row carries its integer fields, and its CRCs, its calls or its message
        assert set(tool.INT_FIELDS) <= set(want)
        if rid.startswith("ed-"):
            assert "calls" in want
        elif rid.startswith("retry-"):
            assert want["status"] == 3 and {"message", "crc32_qhat"} <= set(want) and want["draws"] == 5
        else:
            assert {"crc32_qhat", "crc32_blks"} <= set(want) if want["status"] == 0 else "message" in want
    inst = tool.instances(problems, golden)
    bad = []
    for row in rows:
        got, want = tool.run_row(pkg, inst, row), recorded[row[0]]
        if {k: got.get(k) for k in want} != want:
            bad.append((row[0], got, want))
    assert not bad, bad
