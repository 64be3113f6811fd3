"""Phase probe of k_extend_add and k_big_schur64_ea (ipc_amd/csrc/mf_numeric.hip, -DMF_EA_PROBE): builds the probe library beside the product one and
prints how to run it.  The probe library stamps the wall clock in thread 0 of every workgroup of the two kernels during factorisation 20 of a process and prints
the per-level averages to stderr in front of factorisation 21, so any run with more than 20 Newton iterations will do:

    python tools/ea_gather_probe.py                       # build ipc_amd/libipcgpu_eaprobe.so (hipcc, no GPU needed)
    IPCGPU_LIB_VARIANT=eaprobe python bench.py --steps 40 --warmup 5 --no-cpu-baseline --no-contact --no-large 2> phases.txt

Record: profiles/extend_add_gather_phases.txt."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ipc_amd import build  # noqa: E402

if __name__ == "__main__":
    print(build.build(verbose=True, variant="eaprobe", extra_flags=["-DMF_EA_PROBE"]))
