"""Every path of the module-compression driver (csrc/compress.cpp) against a table recorded once from the csrc of the commit
that tests/golden/module_paths.json names: tools/record_module_paths.py holds the rows and the one way a row is run."""
import importlib.util
import json
import pathlib

import pytest

pytestmark = pytest.mark.gpu


def _tool():
    path = pathlib.Path(__file__).resolve().parents[1] / "tools" / "record_module_paths.py"
    spec = importlib.util.spec_from_file_location("record_module_paths", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_module_path_matches_the_recorded_table(pkg, problems, golden):
    """instance x seed x one flag through blockDiagonalize, and one sdpsr_jordan_reduce per instance that does not fail: the
    commutative module of the class sums with the saved element and the speculative B2, growth rounds with the second
    orthonormalisation step and the small-host tail, w = 6, the device tail of w = 72 > 64 with its side stream, the rejected
    K17 (module exceeds wmax), the non-symmetric verdict behind the first Gram read-back, the automatic selection at
    n = 1024.  Each row -- status or error code and message, block sizes in order, draw position, host waits, CRC32 of Q_hat
    and of blks -- equals the recorded one.  No row reaches the batched label product
    (launch_label_spmm_multi): er7k8 and sym8k24 grow by one G = 2 round at w = 33 and w = 44 (2 w > 64), the others run only the
    G = 1 invariance round, so the SPMM_ONE_BY_ONE rows equal their flag-0 rows in every field."""
    tool = _tool()
    with open(tool.GOLDEN) as f:
        recorded = json.load(f)["rows"]
    rows = tool.rows()
    assert set(recorded) == {row[0] for row in rows} and len(rows) == 110
    for want in recorded.values():  # every row carries its integer fields, and its CRCs or its message
        assert set(tool.INT_FIELDS) <= set(want)
        assert {"crc32_qhat", "crc32_blks"} <= set(want) if want["status"] == 0 else "message" in want
    inst = tool.instances(problems, golden)
    bad = []
    for row in rows:
        got, want = tool.run_row(pkg, inst, row), recorded[row[0]]
        if {k: got.get(k) for k in want} != want:
            bad.append((row[0], got, want))
    assert not bad, bad
