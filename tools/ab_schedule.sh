# usage (GPU box, repo root): bash tools/ab_schedule.sh [rounds=3]   -> build/ab_schedule/<variant>_<round>.json, one summary line each
# The variants are built first, where there is a compiler, one line per variant:
#   python -c "from zeldaengine_amd import build as b; b.build(out=b.HERE + '/libzv_lw4.so', extra_flags=['-DZR_LIGHT_WAVES=4'])"
#   lw4 / lw6: -DZR_LIGHT_WAVES=4 / 6    prio1 / prio2: -DZR_CAM_PRIORITY=1 / 2    wg8 / wg16: -DZR_TILE_WG_PER_CU=8u / 16u    evcam1: -DZR_EV_CAM_AHEAD_OF_PLAN=1
# Every round runs the default build and then each variant that exists, so that drift of the machine falls on all of them alike.
rounds=${1:-3}
O=build/ab_schedule; mkdir -p $O
for i in $(seq 1 $rounds); do
  for v in base lw4 lw6 prio1 prio2 wg8 wg16 evcam1; do
    if [ $v = base ]; then unset ZELDA_RENDER_LIB; elif [ -f zeldaengine_amd/libzv_$v.so ]; then export ZELDA_RENDER_LIB=$PWD/zeldaengine_amd/libzv_$v.so; else continue; fi
    timeout -k 10 300 python bench.py --gpus 1 --no-cpu-baseline --steps 200 --warmup 10 > $O/${v}_$i.json 2> $O/${v}_$i.err || { echo "$v failed"; tail -5 $O/${v}_$i.err; exit 1; }
    python - $O/${v}_$i.json <<'PY'
import json, sys, os
d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
print(os.path.basename(sys.argv[1]), "value", d["value"], "camera", d.get("value_moving_camera"), "light", d.get("value_moving_light"), "textured", d.get("value_textured"))
PY
  done
done
