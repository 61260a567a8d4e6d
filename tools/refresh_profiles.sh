# bash tools/refresh_profiles.sh OUT_DIR: GPU tests, the full bench line, and the forward's kernel statistics / counter passes into OUT_DIR
set -e
O=${1:?usage: bash tools/refresh_profiles.sh OUT_DIR}
mkdir -p $O
R=$PWD
case $O in /*) ;; *) O=$R/$O ;; esac
timeout -k 10 1000 python -m pytest tests -x -q -m gpu > $O/test.log 2>&1 || true
tail -3 $O/test.log
timeout -k 10 400 python bench.py --full > $O/bench.json 2> $O/bench.err
cd /tmp && export TMPDIR=/tmp
BARGS="--steps 2 --warmup 1 --dtype bf16 --no-cpu-baseline --graph 0 --train-steps 0 --no-glow-variant"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o s -- python3 $R/bench.py --steps 5 --warmup 2 --no-cpu-baseline --graph 0 --train-steps 0 --no-glow-variant > $O/stats.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py $BARGS > $O/pf.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/bench.py $BARGS > $O/pw.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_mfma -- python3 $R/bench.py $BARGS > $O/pm.log 2>&1
cd $R
python tools/pmc_traffic.py $O/pmc_fetch $O/pmc_write $O/pmc_traffic.json
python tools/pmc_mfma.py $O/pmc_mfma $O/pmc_mfma.json
ls $O/stats | head; du -sh $O
find $O -name "*counter_collection.csv" -size +5M -delete; find $O -name "*kernel_trace.csv" -path "*pmc*" -delete
