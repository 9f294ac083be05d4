#!/bin/bash
OUT=${OUT:?folder for the results}; export OUT
mkdir -p $OUT/r04
timeout 600 python -m pytest tests/test_gpu_kernels.py -x -q -m gpu -k "value or histogram or select" > $OUT/r04/values_tests.log 2>&1; grep -E "passed|failed|Error" $OUT/r04/values_tests.log | tail -3
DPH_PROFILE=1 timeout 600 python3 bench.py --full --steps 2 --warmup 1 --cpu-rounds 0 --scan-leg-rounds 0 --dense-leg-rounds 0 --map-leg-repeats 0 > $OUT/r04/setup_prof2.json 2> $OUT/r04/setup_prof2.err; grep "\[setup\]" $OUT/r04/setup_prof2.err | tail -6
python3 -c "
import json; d=json.load(open('$OUT/r04/setup_prof2.json')); print(d['value']/1e6, d['parity'], d['job_breakdown_s']['setup_value_table_kmer_index_slots'])"
