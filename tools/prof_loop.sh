export TMPDIR=/tmp; repo=$PWD; out=$(realpath -m ${1:?usage: bash tools/prof_loop.sh <output dir>}); mkdir -p $out
cd /tmp && rocprofv3 --kernel-trace --stats -d /tmp/rp_loop -o loop -- python $repo/bench.py --full --no-cpu-baseline --no-configs3 --no-pmc > $out/bench.json 2> $out/err.txt
db=$(find /tmp/rp_loop -name "*.db" | head -1)
python $repo/tools/rocprof_summary.py $db $out/stats.csv "loop" > /dev/null
head -14 $out/stats.csv | cut -c1-150
python - <<PY
import sqlite3
db = sqlite3.connect("$db")
names = [r[0] for r in db.execute("select name from sqlite_master where type in ('table','view')")]
print([n for n in names if 'kernel' in n.lower()][:20])
PY
