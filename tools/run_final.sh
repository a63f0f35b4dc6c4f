# Round-end measurement set (from the repo root): profile, the full bench line, per-shape table, phase events, every bench line
#   bash tools/run_final.sh <tag>     -> $OUT_DIR (default results/)/<tag>_*; the PMC traffic profile is also copied to profiles/
cd "$(dirname "$0")/.."
tag=${1:-r03}
export OUT_DIR=${OUT_DIR:-$PWD/results}
out=$OUT_DIR
mkdir -p $out
bash tools/profile_step.sh $tag > $out/${tag}_profile.log 2>&1
# the bench line looks its `traffic` up in the newest profiles/*_pmc_traffic.json taken from the SAME kernel sources: the one just made
cp $out/${tag}_pmc_traffic.json profiles/${tag}_pmc_traffic.json
timeout 900 python bench.py --full --gemm-shapes $out/${tag}_gemm_shapes.txt --hbm-shapes $out/${tag}_hbm_shapes.txt > $out/${tag}_bench_B32_1gpu.json 2> $out/${tag}_bench_err.txt
timeout 300 python tools/probe/phase_events.py 32 > $out/${tag}_phase_events.txt 2>&1
timeout 300 python tools/mesh_bench.py 32 2>&1 | grep -v "^W\|amdgpu.ids" > $out/${tag}_mesh_bench.txt
for a in "f32 32" "bf16 32" "bf16 64"; do timeout 250 python3 tools/host_time.py $a 2>&1 | grep -v "^W\|amdgpu.ids" | tail -4; done > $out/${tag}_host_time.txt 2>&1
timeout 300 python3 tools/op_census.py 2>&1 | grep -v "^W\|amdgpu.ids" > $out/${tag}_op_census.txt
timeout 300 python bench.py --config rgb-encoder --no-cpu-baseline > $out/${tag}_bench_rgb_encoder_B8.json 2>/dev/null
timeout 300 python bench.py --full --batch 8 --no-cpu-baseline --no-mpjpe --no-collective-path > $out/${tag}_bench_B8_1gpu.json 2>/dev/null
timeout 300 python bench.py --full --dtype bf16 --batch 32 --steps 30 --warmup 10 --no-cpu-baseline --no-mpjpe > $out/${tag}_bench_bf16_B32_1gpu.json 2>/dev/null
timeout 300 python bench.py --full --dtype bf16 --batch 64 --steps 30 --warmup 10 --no-cpu-baseline --no-mpjpe > $out/${tag}_bench_bf16_B64_1gpu.json 2>/dev/null
tail -c 1500 $out/${tag}_bench_B32_1gpu.json | head -c 600; echo
python - <<PY
import json
d = json.loads(open('$out/${tag}_bench_B32_1gpu.json').read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['kernel'], d['roofline']['achieved'], d['roofline']['frac'], d['roofline']['traffic'])
print(d['roofline']['all_gemm_kernels']['achieved'], d['roofline']['step_level'])
print({k: (v['images_per_s'], v['ms_per_step']) for k, v in d['bf16_per_gpu'].items() if isinstance(v, dict)})
print(d['cpu_baseline'])
PY
