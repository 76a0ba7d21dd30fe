"""GPU: the shadow-8 scan through the pipelined search (ShardedSearch.submit: scan stream, tail stream, ping-pong
workspaces), which only the benchmark ran so far, at every working point of its spare-CU count (hr_index.hip:
tail_cus; DESIGN 3 "Tail stream").

1.2M x 64 bf16 cosine rows are 37,500 tiles: 18 or more per wave on any launch, and enough for the early SAMPLE where
the plan leaves it CUs.  Six batches of 64 queries (half near neighbours, half isotropic) go in back to back at k = 10
and k = 40, then 300k x 1024 with two near-duplicates of every query planted in row parts 0 and 2, so thresholds cross
parts while batches overlap.  Every batch's rows and fp32 score bits must be the oracle's over the stored rows, every
batch must have run the shadow-8 FILTER, and no query may have gone to the collect pass.

The counts are read when the library loads, so each setting runs tests/shadow8_pipelined_child.py in a fresh process;
the oracle's answers are computed once here and handed over in a file.  No setting launches helper workgroups (not in
the tree: DESIGN 7), so there is no per-wave tile sum to check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N64, N1024, NB, B = 1_200_000, 300_000, 6, 64


def make_queries(rng, n, dim, nq, noise):
    """As tests/test_gpu_shadow8_cadence.py: half near neighbours of corpus rows, half isotropic."""
    planted = np.concatenate([R.gen_rows(1, int(j), 1, dim) for j in rng.choice(n, nq, replace=False)])
    q = planted + rng.standard_normal((nq, dim)).astype(np.float32) * noise
    q[1::2] = rng.standard_normal((nq // 2, dim))
    return q.astype(np.float32)


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    rng = np.random.default_rng(11)
    stored = oracle.c_build_synthetic(1, 0, N64, 64, "bf16", "cosine")
    q64 = make_queries(rng, N64, 64, NB * B, 20000)
    s64, r64 = oracle.c_search(stored, "bf16", R.process_queries(q64, "cosine"), 40)
    del stored
    # D = 1024: the last case of tests/shadow8_lds_child.py; one oracle answer for 64 queries, the six batches are
    # permutations of them (each batch meets the table in another order)
    rng = np.random.default_rng(5)
    dim, a, b = 1024, 40_000, 200_000
    q = make_queries(rng, N1024, dim, B, 20000)
    sd = q.std(axis=1, keepdims=True)
    dup_a = (q + rng.standard_normal(q.shape).astype(np.float32) * 0.05 * sd).astype(np.float32)
    dup_b = (q + rng.standard_normal(q.shape).astype(np.float32) * 0.07 * sd).astype(np.float32)
    n_syn = N1024 - 2 * B
    stored = np.concatenate([
        oracle.c_build_synthetic(1, 0, a, dim, "bf16", "cosine"),
        oracle.c_quantize(oracle.c_normalize_rows(dup_a), "bf16"),
        oracle.c_build_synthetic(1, a, b - a, dim, "bf16", "cosine"),
        oracle.c_quantize(oracle.c_normalize_rows(dup_b), "bf16"),
        oracle.c_build_synthetic(1, b, n_syn - b, dim, "bf16", "cosine")])
    assert stored.shape[0] == N1024
    s, r = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), 10)
    del stored
    want = np.stack([a + np.arange(B), b + B + np.arange(B)], axis=1)
    assert np.array_equal(np.sort(r[:, :2], axis=1), want)  # the duplicates lead every answer
    perms = [np.arange(B)] + [rng.permutation(B) for _ in range(NB - 1)]
    path = str(tmp_path_factory.mktemp("shadow8_pipelined") / "ref.npz")
    np.savez(path, n64=N64, q64=q64.reshape(NB, B, 64), s64=s64.reshape(NB, B, 40), r64=r64.reshape(NB, B, 40),
             dup_a_at=a, dup_b_at=b, n_syn=n_syn, dup_a=dup_a, dup_b=dup_b,
             q1024=np.stack([q[p] for p in perms]), s1024=np.stack([s[p] for p in perms]),
             r1024=np.stack([r[p] for p in perms]))
    return path


# the default (the shadow-8 plan takes every CU, the 16-bit scans leave 32), the shadow-8 plan at the 16-bit scans'
# count (early SAMPLE beside the previous FILTER) and at 8 (an early SAMPLE of 8 workgroups), and no spare CU anywhere
SETTINGS = [{}, {"HIPRAG_TAIL_CUS8": "32"}, {"HIPRAG_TAIL_CUS8": "8"}, {"HIPRAG_TAIL_CUS": "0"}]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "defaults")
def test_pipelined_shadow8_batches_equal_the_oracle(reference, setting):
    env = {k: v for k, v in os.environ.items() if k not in ("HIPRAG_TAIL_CUS", "HIPRAG_TAIL_CUS8")}
    env.update(setting)
    p = subprocess.run([sys.executable, os.path.join(HERE, "shadow8_pipelined_child.py"), reference], env=env,
                       capture_output=True, text=True, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(lines[-1])
    for case in res["cases"]:
        print(case)
    assert res["ok"], res
    assert res["env"] == {k: setting.get(k) for k in ("HIPRAG_TAIL_CUS", "HIPRAG_TAIL_CUS8")}, res
    assert len(res["cases"]) == 3, res
    for c in res["cases"]:
        assert c["launches"] == c["batches"] == NB, c
        assert c["guard_failures"] == 0 and c["fallback_queries"] == 0, c
        assert all(c["rows_equal"]) and all(c["score_bits_equal"]), c
