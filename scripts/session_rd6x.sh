#!/bin/bash
# round 6 check after the DEQ / attention changes (Skip DEQ-CIFAR preset, Anderson adjoint option,
# attention forward LDS layout): whole GPU suite, smoke(), bench lines, DEQ-CIFAR --force-comm steady trace
source "$(dirname "$0")/gpu_lib.sh"
rm -f "$OUT/steps.log" "$OUT/bench_results.jsonl"
export HSA_ENABLE_IPC_MODE_LEGACY=0
step pytest_gpu 1000 0 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider
step smoke 200 0 python -c "import __graft_entry__ as g; g.smoke()"
B="python bench.py --steps 20 --warmup 10"
step resnet 300 0 python bench.py
step vit 300 0 $B --model vit_b16
step deq 300 0 $B --model deq
step deq_cifar 300 0 $B --model deq_cifar
step deq_cifar_comm 300 0 $B --model deq_cifar --force-comm
cd /tmp
step prof_deqc 300 0 rocprofv3 --kernel-trace --stats -d "$OUT/prof_deqc_rd6x" -o run --output-format csv -- \
  python3 "$ROOT/bench.py" --model deq_cifar --force-comm --full --steps 5 --warmup 5
cd "$ROOT"
echo done
