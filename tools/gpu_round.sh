# Round-end style GPU session: tests, full bench (with CPU baseline + recall), smoke, profiles.
# Every GPU step has its own time limit; the first failure ends the session.  Logs go to $OUT (default bench_out/).
set -u
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests/ -x -q -m gpu --timeout 120 --timeout-method thread -rf > "$OUT/t_all.log" 2>&1; rc=$?
echo "pytest rc=$rc"; tail -3 "$OUT/t_all.log"
[ $rc -ne 0 ] && exit $rc
timeout -k 10 600 python -u bench.py --full > "$OUT/bench_full.log" 2>&1; rb=$?
echo "bench rc=$rb"; tail -1 "$OUT/bench_full.log"
[ $rb -ne 0 ] && exit $rb
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1; rs=$?
echo "smoke rc=$rs"; tail -1 "$OUT/smoke.log"
[ $rs -ne 0 ] && exit $rs
[ "${NO_PROFILE:-0}" = 1 ] && exit 0
bash tools/profile.sh ${1:-r01}
