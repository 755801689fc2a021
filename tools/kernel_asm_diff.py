"""Compare the device code of kernels between two builds: python tools/kernel_asm_diff.py OLD.s NEW.s REGEX
Each .s is the device assembly of a translation unit, e.g.
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC --offload-device-only -S -o new.s bayesianlinearregressors.jl_amd/csrc/blr_abi.hip
For every kernel of OLD.s whose mangled name matches REGEX, the instructions and kernel descriptor are compared with those of the
same kernel in NEW.s, after dropping comments and renumbering local labels.  A kernel that gained a defaulted template parameter
(marginals_gemm_kernel<T, ROWV, A = MarginalArgs<T>>) is matched by its demangled name without it, and the symbol
names themselves are left out of the comparison.  Exit status 1 if any kernel differs or is missing."""
import re
import subprocess
import sys


def functions(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
                continue
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
            line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
            line = line.split(";")[0].rstrip().replace(name, "@KERNEL")  # (the descriptor and section lines name the kernel)
            if line.strip():
                cur.append(line)
    return out, descriptors(path)


def descriptors(path):
    """.amdhsa_kernel blocks by kernel name (register counts, LDS, scratch)"""
    out, cur, name = {}, None, None
    for line in open(path):
        s = line.strip()
        if s.startswith(".amdhsa_kernel "):
            name, cur = s.split()[1], []
        elif s.startswith(".end_amdhsa_kernel") and cur is not None:
            out[name] = cur
            cur = None
        elif cur is not None:
            cur.append(s.replace(name, "@KERNEL"))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[: len(names)]


def key(dm):
    """demangled name without a defaulted MarginalArgs template argument and without the return type / parameter list"""
    dm = re.sub(r", blr::MarginalArgs<(double|float)> >", ">", dm)
    dm = re.sub(r"^void ", "", dm)
    dm = dm.replace("(anonymous namespace)::", "")  # (its parenthesis is not the parameter list's: mean_small_kernel<double> / <float>)
    return dm.split("(")[0]


def main():
    old_path, new_path, pat = sys.argv[1], sys.argv[2], re.compile(sys.argv[3])
    (fo, do), (fn, dn) = functions(old_path), functions(new_path)
    old = sorted(n for n in fo if pat.search(n))
    new_names = sorted(fn)
    by_key = dict(zip((key(d) for d in demangle(new_names)), new_names))
    bad = 0
    for n, dm in zip(old, demangle(old)):
        m = by_key.get(key(dm))
        if m is None:
            print("MISSING", dm)
            bad += 1
            continue
        same = fo[n] == fn[m] and do.get(n) == dn.get(m)
        bad += not same
        print("SAME" if same else "DIFF", f"{len(fo[n]):6d} lines", dm, "" if m == n else f"(now {m})")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
