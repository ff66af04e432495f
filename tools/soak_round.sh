# the round's soaks in one GPU session: tools/soak_round.sh OUTDIR  ->  OUTDIR/*.log, *.out, *.err
O=${1:?usage: tools/soak_round.sh OUTDIR}; mkdir -p $O
python -m pytest tests/test_gpu_parity.py -q -k "pinning_that_covers or pinned" > $O/pin.log 2>&1; tail -3 $O/pin.log
# N > 1 control flow at real sizes: 4 ranks on one GPU at the full shape, 8 at a quarter of the tiles; --full for the fan-in and the per-rank check
python bench.py --gpus 4 --oversubscribe --steps 3 --warmup 1 --full > $O/n4.out 2> $O/n4.err; echo "rc=$?" >> $O/n4.err
python bench.py --gpus 8 --oversubscribe --tiles 98304 --steps 3 --warmup 1 --full > $O/n8.out 2> $O/n8.err; echo "rc=$?" >> $O/n8.err
MDEMOD_BENCH_FAULT=fanin_hang@3 MDEMOD_BENCH_POST_DEADLINE_S=60 python bench.py --gpus 4 --oversubscribe --tiles 98304 --steps 2 --warmup 1 --full > $O/n4hang.out 2> $O/n4hang.err; echo "rc=$?" >> $O/n4hang.err
wc -c $O/*.out; tail -c 300 $O/n4.err
# soaks on the round's build, fresh seeds
S=$(date +%s)
python tools/config_fuzz.py 1500 $S > $O/config_fuzz.log 2>&1; tail -2 $O/config_fuzz.log
FUZZ_HYB=1 python tools/config_fuzz.py 400 $((S+1)) > $O/config_fuzz_hyb.log 2>&1; tail -2 $O/config_fuzz_hyb.log
python tools/api_fuzz.py 1500 $((S+2)) > $O/api_fuzz.log 2>&1; tail -2 $O/api_fuzz.log
python tools/recording_fuzz.py 200 $((S+3)) > $O/recording_fuzz.log 2>&1; tail -3 $O/recording_fuzz.log
python tools/cli_fuzz.py 250 $((S+4)) > $O/cli_fuzz.log 2>&1; tail -2 $O/cli_fuzz.log
python tools/recording_opts_fuzz.py 100 $((S+5)) > $O/recording_opts_fuzz.log 2>&1; tail -2 $O/recording_opts_fuzz.log
