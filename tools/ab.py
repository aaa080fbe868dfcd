"""Same-box A/B measurements of kernel variants (the GPU boxes of the pool differ by up to 8 % on identical code, so a
variant is only ever compared with the baseline inside ONE gpurun call).

1. here (no GPU needed, hipcc cross-compiles):
       python tools/ab.py build base  rb8:-DMK_FFT_RB1440=8  nt256:-DMK_FFT_NT1440=256
   builds makani_amd/libmakani_amd_<tag>.so for every `tag[:-Dmacro=value,...]` (the kernel source must read the macro);
2. on the GPU box, inside one gpurun call:
       python tools/ab.py run [--timeout SECONDS] [--repeat N] base rb8 nt256 -- python tools/microbench.py fft
   runs the command once per variant with MAKANI_AMD_LIB pointing at it and prints the outputs side by side.  A variant that
   exits non-zero or runs past its time limit (default 600 s per variant, sized for tools/microbench.py) is the LAST one
   started: after a fault nothing more may touch the GPU, so the outputs so far are printed and ab.py exits with that status.
   An arm may carry environment settings, `tag@VAR=VALUE[,VAR=VALUE]` (a path that Python, not a macro, selects:
   `parent@MAKANI_AMD_NORM1_FOLD=0 new`), and `--repeat N` runs the arms N times in alternation (parent new parent new: drift of
   the box over the call hits both arms alike); the outputs are labelled `tag#k`.
`base` without defines is the default library rebuilt under its own tag, so that all variants come from the same sources."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lib_of(tag):
    return os.path.join(ROOT, "makani_amd", f"libmakani_amd_{tag}.so")


def build(specs):
    from makani_amd import build as mb
    for spec in specs:
        tag, _, defs = spec.partition(":")
        path = mb.build(defines=[d for d in defs.split(",") if d], tag=tag, verbose=False)
        print(f"{tag}: {path}")


def run(arms, cmd, timeout=600.0, repeat=1):
    specs = []
    for arm in arms:
        tag, _, envs = arm.partition("@")
        if not os.path.exists(lib_of(tag)):
            raise SystemExit(f"{lib_of(tag)} is missing: run `python tools/ab.py build {tag}[:-D...]` first")
        specs.append((tag, dict(e.split("=", 1) for e in envs.split(",") if e)))
    runs = [(tag if repeat == 1 else f"{tag}#{k + 1}", tag, env) for k in range(repeat) for tag, env in specs]
    outs, status = {}, 0
    for label, tag, env in runs:
        try:
            r = subprocess.run(cmd, env=dict(os.environ, MAKANI_AMD_LIB=lib_of(tag), **env), capture_output=True, text=True, timeout=timeout)
            text, status = r.stdout + r.stderr, r.returncode
        except subprocess.TimeoutExpired as e:                 # (subprocess.run has killed and reaped the child)
            text = "".join(t.decode(errors="replace") if isinstance(t, bytes) else t for t in (e.stdout, e.stderr) if t)
            status = 124
        outs[label] = [l for l in text.splitlines() if l.strip() and "amdgpu.ids" not in l]
        if status:
            print(f"[{label}] {'ran past its time limit of %g s' % timeout if status == 124 else 'exit code %d' % status}: "
                  f"not starting {[l for l, _, _ in runs if l not in outs] or 'anything else'}")
            break
    n = max(len(v) for v in outs.values())
    for i in range(n):
        for label in outs:
            line = outs[label][i] if i < len(outs[label]) else ""
            print(f"{label:>10s} | {line}")
        print()
    return status


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] not in ("build", "run"):
        raise SystemExit(__doc__)
    if sys.argv[1] == "build":
        build(sys.argv[2:])
    else:
        args = sys.argv[2:sys.argv.index("--")]
        limit, repeat = 600.0, 1
        while args and args[0] in ("--timeout", "--repeat"):
            if args[0] == "--timeout":
                limit = float(args[1])
            else:
                repeat = int(args[1])
            args = args[2:]
        sys.exit(run(args, sys.argv[sys.argv.index("--") + 1:], limit, repeat))
