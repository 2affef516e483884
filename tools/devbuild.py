"""Kernel-tuning build: the named .hip files recompiled with the given -D flags (source list and hipcc line: ppca_rs_amd.build)
and linked with the current objects of all the other sources into ppca_rs_amd/libppca_hip_<name>.so (select it with PPCA_HIP_LIB).
    python tools/devbuild.py --name=dev ppca_kernels.hip ppca_pass.hip ppca_em9.hip ppca_llk.hip -DPPCA_DEV_K10   (the fused kernels for k = 10 only)
    python tools/devbuild.py --name=dev16 ppca_em16.hip -DPPCA_E16_ONLY=16
    python tools/devbuild.py --name=pipe0 ppca_generic.hip -DI8_PIPE=0
`--timing` adds -DPPCA_PHASE_TIMING and recompiles ppca_capi.hip too (it prints the phase table); `--asm` also leaves each
named file's device listing, csrc/<file>.<name>.s."""
import os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppca_rs_amd import build as B
args, timing = sys.argv[1:], "--timing" in sys.argv
name = ([a.split("=", 1)[1] for a in args if a.startswith("--name=")] or ["dev"])[0]
mine = [a for a in args if a.endswith(".hip")] + (["ppca_capi.hip"] if timing and "ppca_capi.hip" not in args else [])
assert mine and all(f in B.SOURCES for f in mine), "name the .hip files to recompile, out of: " + " ".join(B.SOURCES)
path = lambda src, ext: os.path.join(B.CSRC, src.replace(".hip", ext))
B.build(force=not all(os.path.exists(path(f, ".o")) for f in B.SOURCES if f not in mine))  # the others' objects: what is out of date; all, if one is missing
base = [B._hipcc(), *B.FLAGS, *[a for a in args if a.startswith("-D")], *(["-DPPCA_PHASE_TIMING"] if timing else [])]
procs = [subprocess.Popen(base + ["-c", path(f, ".hip"), "-o", path(f, ".%s.o" % name)]) for f in mine]
if "--asm" in args:
    procs += [subprocess.Popen(base + ["--offload-device-only", "-S", path(f, ".hip"), "-o", path(f, ".%s.s" % name)], stderr=subprocess.DEVNULL) for f in mine]
assert all(p.wait() == 0 for p in procs)
out = os.path.join(B.HERE, "libppca_hip_%s.so" % name)
subprocess.check_call(base[:2] + ["-shared", "-fPIC", "-o", out] + [path(f, ".%s.o" % name if f in mine else ".o") for f in B.SOURCES])
print(out)
