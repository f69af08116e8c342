"""Developer tool: prove that a change to cdfo_amd/csrc changed no kernel's instructions.

    python tools/isa_diff.py REV [--dev] [-j N] [--by-kernel]

Unpacks REV with `git archive`, compiles every csrc/*.hip of that tree and of the working tree to device assembly (build.py's
FLAGS plus -S --cuda-device-only; --dev adds -DCDFO_DEV_ABLATIONS), drops the lines that name the per-file __hip_cuid_ symbol
(hipcc derives it from the file's path and text: the only thing that differs between two equal compilations) and prints a unified
diff per file, or `identical`.  Exit status 1 on any difference.

--by-kernel: for a change that ADDS instantiations to a file (which renumbers every label behind them and may rename the existing
kernels' symbols): every kernel of REV must be found in the working tree's file with the same instructions -- basic-block labels
without their function number, comments dropped, the kernel's own symbol masked.  Prints per file how many of REV's kernels were
found and how many the working tree adds; exit status 1 if one is missing."""
import argparse, concurrent.futures as cf, difflib, importlib.util, io, os, re, subprocess, sys, tarfile, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_JOBS = 16


def _build_py():
    spec = importlib.util.spec_from_file_location("cdfo_build", os.path.join(ROOT, "cdfo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def normalise(asm):
    """assembly text -> its lines without those that name the __hip_cuid_ symbol"""
    return [l for l in asm.split("\n") if "__hip_cuid_" not in l]


def diff(name, old, new):
    """unified diff (a list of lines, empty when equal) of two assembly texts of csrc file `name`"""
    return list(difflib.unified_diff(normalise(old), normalise(new), "a/" + name, "b/" + name, lineterm="", n=3))


def kernels(asm):
    """assembly text -> {symbol: its instructions as one string}, labels, comments and the symbol itself normalised (--by-kernel)"""
    res = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.S | re.M):
        body = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))
        body = "\n".join(l.split(";")[0].rstrip() for l in body.split("\n") if "__hip_cuid_" not in l)
        res[m.group(1)] = body.replace(m.group(1), "KERNEL")
    return res


def missing_kernels(old, new):
    """(symbols of `old` whose instructions no kernel of `new` has, kernels of `old`, kernels `new` adds)"""
    o, n = kernels(old), kernels(new)
    have = set(n.values())
    return [k for k, v in o.items() if v not in have], len(o), len([k for k, v in n.items() if v not in set(o.values())])


def _assemble(hipcc, flags, src, out):
    r = subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", "-o", out, src], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr[-2000:]}")
    return open(out).read()


def assemble_tree(tree, outdir, flags, hipcc, ex):
    """{file name: future of its assembly text} for every csrc/*.hip under the checkout at `tree`"""
    csrc = os.path.join(tree, "cdfo_amd", "csrc")
    os.makedirs(outdir, exist_ok=True)
    return {f: ex.submit(_assemble, hipcc, flags, os.path.join(csrc, f), os.path.join(outdir, f[:-4] + ".s"))
            for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev")
    ap.add_argument("--dev", action="store_true", help="compile with -DCDFO_DEV_ABLATIONS")
    ap.add_argument("-j", type=int, default=8, dest="jobs")
    ap.add_argument("--by-kernel", action="store_true", help="every kernel of REV is still there with the same instructions")
    a = ap.parse_args(argv)
    b = _build_py()
    flags = b.FLAGS + (["-DCDFO_DEV_ABLATIONS"] if a.dev else [])
    with tempfile.TemporaryDirectory() as td:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, "cdfo_amd/csrc", "include"], capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(td, "old"))
        with cf.ThreadPoolExecutor(max_workers=max(1, min(a.jobs, MAX_JOBS))) as ex:
            old = assemble_tree(os.path.join(td, "old"), os.path.join(td, "old_s"), flags, b.HIPCC, ex)
            new = assemble_tree(ROOT, os.path.join(td, "new_s"), flags, b.HIPCC, ex)
            differ = 0
            for f in sorted(set(old) | set(new)):
                if f not in old or f not in new:
                    print(f"{f}: only in {'the working tree' if f in new else a.rev}")
                    differ += 1
                    continue
                if a.by_kernel:
                    gone, n_old, n_add = missing_kernels(old[f].result(), new[f].result())
                    print(f"{f}: {n_old - len(gone)} of {n_old} kernels unchanged, {n_add} added" + "".join(f"\n  changed or gone: {k}" for k in gone))
                    differ += bool(gone)
                    continue
                d = diff(f, old[f].result(), new[f].result())
                print(f"{f}: identical" if not d else "\n".join(d))
                differ += bool(d)
    print(f"{differ} file(s) differ from {a.rev}" if differ else f"all {len(new)} files identical to {a.rev}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
