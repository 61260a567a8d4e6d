# A/B of one environment switch on the forward bench (and optionally the train step): bash tools/ab_env.sh OUT_DIR VAR "0 1" [train]
# two rounds per value, same box.  Output: OUT_DIR/ab_<VAR>.log
O=${1:?usage: bash tools/ab_env.sh OUT_DIR VAR VALUES [train_steps]}; V=$2; VALS=$3; TR=${4:-0}
mkdir -p $O
L=$O/ab_$V.log
: > $L
for r in 1 2; do for v in $VALS; do
  env $V=$v timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-glow-variant --train-steps $TR > $O/ab_tmp.json 2> $O/ab_tmp.err || { tail -5 $O/ab_tmp.err; exit 1; }
  python - $V $v $O/ab_tmp.json >> $L <<'PY'
import json,sys
d=json.loads(open(sys.argv[3]).read().strip().splitlines()[-1])
t=d.get('train_step') or {}
print(sys.argv[1], sys.argv[2], 'fwd', d['ms_per_step'], 'train', t.get('ms_per_step'))
PY
done; done
cat $L
