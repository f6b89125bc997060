"""Holds a refactor of the kernel sources to "no kernel's instructions change": compiles every unit of this tree and of a base
revision for gfx950 with its build.py flags and compares, kernel by kernel, the instruction stream and the .amdhsa_
descriptor (registers, LDS, scratch).  Needs hipcc and git only, no GPU.

    python tools/isa_compare.py [BASE_REV, default HEAD] > profiles/<change>_isa_compare.txt      (exit status 1 = a difference)
"""
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(root):
    """{kernel symbol: (unit, instruction lines, descriptor lines)} of the tree at root"""
    spec = importlib.util.spec_from_file_location("build_of_" + str(abs(hash(root))), os.path.join(root, "codlad_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)

    def unit(s):
        cmd = [b.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + b.EXTRA_FLAGS.get(s, []) + \
              ["--cuda-device-only", "-S", "-o", "-", os.path.join(b.CSRC, s)]
        asm = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
        asm = re.sub(r";.*", "", asm)                                  # comments
        # local labels are numbered by a kernel's position in its unit
        asm = re.sub(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+", r".\1N", asm)
        lines = lambda text: [ln.strip() for ln in text.splitlines() if ln.strip()]
        found = {}
        for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M):
            # <name>: instructions, .amdhsa_kernel <name>, descriptor, .end_amdhsa_kernel
            body, desc = re.search(r"^%s:[ \t]*\n(.*?)\.amdhsa_kernel %s[ \t]*\n(.*?)\.end_amdhsa_kernel"
                                   % (re.escape(name), re.escape(name)), asm, re.M | re.S).groups()
            found[name] = (s, lines(body), lines(desc))
        return found

    out = {}
    with concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 4, len(b.SOURCES))) as pool:
        for found in pool.map(unit, b.SOURCES):
            assert not set(found) & set(out), "a kernel symbol in two units: %s" % (set(found) & set(out))
            out.update(found)
    return out


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    with tempfile.TemporaryDirectory() as base:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "codlad_amd", "include"], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", base], input=tar, check=True)
        old, new = kernels(base), kernels(ROOT)
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], check=True, stdout=subprocess.PIPE, text=True).stdout.strip()
    print(f"# gfx950 kernels of the working tree against {sha}: instructions and .amdhsa_ descriptor, kernel by kernel")
    bad = 0
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        if not o or not n:
            verdict = "ONLY IN BASE" if o else "ONLY IN TREE"
        else:
            verdict = "same" if o[1:] == n[1:] else "DIFFERENT " + ("instructions" if o[1] != n[1] else "descriptor")
        bad += verdict != "same"
        u = (o or n)[0] if not (o and n) or o[0] == n[0] else f"{o[0]} -> {n[0]}"
        print(f"{verdict:9s} {len((n or o)[1]):6d} lines  {name}  [{u}]")
    print(f"# {len(new)} kernels, {bad} not the same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
