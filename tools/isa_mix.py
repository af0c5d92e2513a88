"""Static instruction mix of a step-kernel instance from `hipcc -S` output (build container).
usage: python tools/isa_mix.py [G DEG MULTI WIDE [dead]] (default 64 2 0 0; `dead`: the instance's state-only twin); writes the
kernel's ISA to /tmp/kernel_<...>.s"""
import re, subprocess, sys, os
from collections import Counter
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
key = tuple(sys.argv[1:5]) if len(sys.argv) >= 5 else ("64", "2", "0", "0")
extra = sys.argv[5:]
dead = "1" if extra[:1] == ["dead"] else "0"
extra = extra[1:] if dead == "1" else extra
subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-mllvm", "-disable-machine-licm",
                "-mllvm", "-amdgpu-kernarg-preload-count=12", "-mllvm", "-amdgpu-sched-strategy=max-memory-clause", "-S", "--cuda-device-only", *extra,
                os.path.join(ROOT, "fleetrl_amd/csrc/fleet_kernels.hip"), "-o", "/tmp/k.s"], check=True, stderr=subprocess.DEVNULL)
lines = open("/tmp/k.s").read().split("\n")
start = None
for i, l in enumerate(lines):
    m = re.match(r"_ZN12_GLOBAL__N_117fleet_step_kernelILi(\d+)ELi(\d)ELb(\d)ELb(\d)ELb\dELb0ELi\dELb(\d)E\w*:", l)
    if m and m.groups() == key + (dead,):  # (the first such instance with float32 actions, A64 = 0)
        start = i
        break
assert start is not None, key
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[start:end]
open("/tmp/kernel_%s.s" % "_".join(key + (("dead",) if dead == "1" else ())), "w").write("\n".join(body))
ins = [l.strip().split()[0] for l in body if l.startswith("\t") and not l.strip().startswith((".", ";"))]
c = Counter()
for x in ins:
    if x.startswith("v_"):
        k = "v_*_f64" if "f64" in x else "v_cmp" if x.startswith("v_cmp") else "v_cndmask" if "cndmask" in x else "v_mov" if "mov" in x else "v_other"
    elif x.startswith("s_"):
        k = "s_waitcnt" if "waitcnt" in x else "s_branch" if ("branch" in x or "cbranch" in x) else "s_other"
    elif x.startswith(("global_", "buffer_", "flat_", "scratch_")):
        k = "vmem_load" if "load" in x else "vmem_store"
    else:
        k = "other"
    c[k] += 1
print(key + (("dead",) if dead == "1" else ()), "static instructions:", len(ins), dict(c))
