# Host-path A/B of two builds of the library with the same kernels (a host-code refactor): the
# parent's libtfhe_gpu.so against this tree's, alternating, REPS times each, in one call on one GPU.
#   bash tools/host_ab.sh PARENT_LIB [REPS] [OUT] [what ...]
# what: nand (the default bench.py line), reenc and adder (bench.py workloads with a host_buffers
# figure: tfhe_gpu_reencrypt_batch, tfhe_gpu_circuit_eval), lookup, packed, lutcirc (the three
# tools at their defaults); default all six.  Every run is a fresh process under its own time limit,
# the first failure ends the script.  OUT (default build/host_ab, relative to the repository root)
# receives the result lines, <what>.<lib>.<rep>.json, and summary.txt: the table of every run and
# the verdicts (branch median against the parent's min-to-max range).
set -o pipefail
PARENT=$(realpath "${1:?parent library}")
REPS=${2:-3}
OUT=${3:-build/host_ab}
shift; shift; shift
WHATS=${*:-nand reenc adder lookup packed lutcirc}
cd "$(dirname "$0")/.."
BRANCH=$PWD/zig-tfhe_amd/lib/libtfhe_gpu.so
mkdir -p $OUT
[ -f "$PARENT" ] && [ -f $BRANCH ] || { echo "library missing"; exit 2; }
for rep in $(seq 1 $REPS); do
  [ $((rep % 2)) = 1 ] && order="parent branch" || order="branch parent"  # neither always runs on the warmer GPU
  for name in $order; do
    [ $name = parent ] && lib=$PARENT || lib=$BRANCH
    for what in $WHATS; do
      case $what in
      nand)    cmd="python bench.py --gpus 1 --steps 50 --warmup 3" ;;
      reenc)   cmd="python bench.py --workload reenc --batch 16384 --steps 8 --warmup 1" ;;
      adder)   cmd="python bench.py --workload adder --batch 1 --steps 5 --warmup 1" ;;
      lookup)  cmd="python tools/lookup_bench.py" ;;
      packed)  cmd="python tools/packed_lookup_bench.py" ;;
      lutcirc) cmd="python tools/lut_circuit_bench.py" ;;
      *) echo "unknown benchmark $what"; exit 9 ;;
      esac
      f=$OUT/$what.$name.$rep
      TFHE_GPU_LIB=$lib timeout -k 10 240 $cmd > $f.json 2> $f.err || { rc=$?; echo "$what $name $rep failed ($rc)"; tail -5 $f.err; exit $rc; }
      echo "$what $name $rep ok"
    done
  done
done
python - $OUT $REPS $WHATS > $OUT/summary.txt <<'EOF' || exit 3
import json, statistics, sys
out, reps, whats = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
def figures(d):  # headline value, then every host-buffer figure of the line
    f = {"value [" + d["unit"] + "]": d["value"]}
    for key in ("host_buffers", "host_buffer"):
        for k, v in d.get(key, {}).items():
            if isinstance(v, (int, float)):
                f[key + "." + k] = v
    return f
print("what / figure: parent runs | branch runs | parent min..max | branch median | verdict")
for what in whats:
    runs = {lib: [figures(json.loads(open(f"{out}/{what}.{lib}.{r}.json").read().strip().splitlines()[-1]))
                  for r in range(1, reps + 1)] for lib in ("parent", "branch")}
    for fig in runs["parent"][0]:
        p, b = [x[fig] for x in runs["parent"]], [x[fig] for x in runs["branch"]]
        med, lo, hi = statistics.median(b), min(p), max(p)
        slower_is_higher = "ms" in fig
        verdict = "inside" if lo <= med <= hi else "outside, faster" if (med < lo) == slower_is_higher else "outside, SLOWER"
        print(f"{what} / {fig}: {p} | {b} | {lo}..{hi} | {med} | {verdict}")
EOF
cat $OUT/summary.txt
