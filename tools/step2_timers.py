"""In-kernel phase timers of k_mbest_step2: build a variant with -DPH_STEP2_TIMERS (hipcc ... -o _var/lib_s2t.so) and run
    PYPERIOD_AMD_LIB=$PWD/_var/lib_s2t.so python3 tools/step2_timers.py
Every 128th workgroup (-DPH_STEP2_TIMERS_EVERY=16: every 16th) prints staging / fold / DMA drain / flush+scan / split /
final flush times (100 MHz ticks), rows examined and splits.  The instrumented kernel is several times slower than the
default build (profiles/step2_chain/README.md): read the table for the shape of a row, not for its microseconds."""
import os, sys
sys.path.insert(0, os.getcwd())
import torch
from pyperiod_amd import PeriodEngine
from pyperiod_amd.synth import multi_sinusoid_batch
eng = PeriodEngine(0)
x = torch.from_numpy(multi_sinusoid_batch(0, 1024, 4096)).cuda()
eng.m_best(x, 10); torch.cuda.synchronize()
print("----")
eng.m_best(x, 10); torch.cuda.synchronize()
