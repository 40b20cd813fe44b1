#!/bin/bash
set -x
cd /root/repo
mkdir -p gpurun_out
{
echo "=== bench (driver contract, 50 steps)"
timeout 600 python bench.py --steps 50 --warmup 5 --full 2>&1 | tail -1
echo "=== gmg 2047^2 / 4095^2 / diffusion"
timeout 600 python examples/gmg.py -k 11 2>&1 | grep solve:
timeout 600 python examples/gmg.py -k 12 2>&1 | grep solve:
timeout 600 python examples/gmg.py -k 10 -d diffusion 2>&1 | grep solve:
echo "=== own pde 4096 throughput"
timeout 600 python examples/pde.py --throughput -i 1000 -w 100 -n 4096 2>&1 | tail -2
echo "=== UNMODIFIED reference pde 4096/8192"
cd examples/upstream
PYTHONPATH=/root/repo timeout 600 python pde.py --package legate -n 4096 -m 4096 -t -i 1000 -w 100 2>&1 | tail -1
PYTHONPATH=/root/repo timeout 900 python pde.py --package legate -n 8192 -m 8192 -t -i 300 -w 50 2>&1 | tail -1
cd /root/repo
echo "=== gmres"
timeout 420 python benchmarks/gmres_timing.py 2>&1 | head -1
echo "=== rmat"
timeout 420 python benchmarks/spgemm_rmat.py --scale 18 --iters 3 2>&1 | tail -1
timeout 900 python benchmarks/spgemm_rmat.py --scale 20 --iters 2 2>&1 | tail -1
} 2>&1 | tee gpurun_out/final_measure.log
