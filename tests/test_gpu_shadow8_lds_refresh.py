"""GPU: the shadow-8 FILTER's shared threshold refresh (scan_body: slice_apply) under a 2-tile cadence.

Each wave of a workgroup refreshes one eighth of the thresholds from the group-max table, shares them through a row
in LDS and publishes its own group maxima where they beat its threshold, not a loaded key.  300,000 rows are 9,375
tiles over at most 2,048 waves, so with HIPRAG_REFRESH_EVERY8=2 every wave refreshes at least twice in mid-scan:
thresholds written by other waves are read back, slices rotate, and the results must still be the oracle's, rows and
score bits, with no query sent to the collect pass.

The cadence and the switch are read when the library loads, so the cases (tests/shadow8_lds_child.py: np = 4 and 5,
QB = 1 and 2, the LDS-full fallback at D = 1280, planted duplicates in two row parts at D = 1024) run in ONE fresh
child process, which stops at its first failure; this test only reads its exit status and its one JSON line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_shared_refresh_keeps_results_exact_at_a_2_tile_cadence():
    env = dict(os.environ, HIPRAG_REFRESH_EVERY8="2", HIPRAG_REFRESH_LDS="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "shadow8_lds_child.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(lines[-1])
    for case in res["cases"]:
        print(case)
    assert res["ok"], res
    assert len(res["cases"]) == 5, res
    assert all(c["ok"] and c["launches"] > 0 and c["guard_failures"] == 0 and c["rows_equal"] and c["scores_equal"]
               for c in res["cases"]), res
