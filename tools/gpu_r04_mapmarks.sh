#!/bin/bash
OUT=${OUT:?folder for the results}; export OUT
mkdir -p $OUT/r04
DPH_PROFILE=1 timeout 600 python3 bench.py --full --steps 1 --warmup 0 --max-rounds 2 --cpu-rounds 0 --scan-leg-rounds 0 --dense-leg-rounds 0 --map-leg-repeats 4 > $OUT/r04/map_marks.json 2> $OUT/r04/map_marks.err
python3 -c "
import json
d=json.loads([l for l in open('$OUT/r04/map_marks.json') if l.startswith('{')][-1])['map_config3']; print(d['value'], d['wall_s_runs'], d['breakdown_s'], d['paf_sha256_matches_oracle_fixture'])"
grep "map setup" $OUT/r04/map_marks.err | tail -7
