cd $GRAFT_REPO_ROOT
timeout 1200 python3 -m pytest tests/test_gpu_train.py tests/test_gpu_plan_mol.py tests/test_dataset_train.py tests/test_graphstep.py -x -q 2>&1 | tail -3
for i in 1 2; do timeout 600 python3 bench.py --full --no-cpu-baseline --no-roofline --no-round3-shapes 2>/dev/null | tail -1 | python3 -c "
import json,sys
d=json.loads(sys.stdin.read()); e=d['epoch_sample']; print(d['value'], d['ms_per_step'], e['ms_per_step_incl_gpu_collate'], e['molecules_per_s_incl_gpu_collate'], e['eager_fallbacks'])"; done
