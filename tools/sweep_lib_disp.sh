# bench every tuning build under gpurun_variants/ on displaced chain starts (IRS_LIB selects the shared library)
J=$(mktemp); E=$(mktemp); trap 'rm -f "$J" "$E"' EXIT   # the bench line / its stderr
for amp in 6 12; do
for f in gpurun_variants/*.so; do
  IRS_LIB=$PWD/$f python bench.py --full --no-cpu-baseline --no-extras --steps 15 --init wave --init-amp $amp "$@" > "$J" 2>"$E" && python -c "
import json,sys;d=json.load(open('$J'));s=d['stage_ms'];print('$f amp $amp',round(d['ms_per_step'],3),'exp_bwd',round(s.get('exp_bwd_ms',0),3),'exp_fwd',round(s.get('exp_fwd_ms',0),3))"
done; done
