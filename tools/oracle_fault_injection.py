#!/usr/bin/env python3
"""Do the float-range tests discriminate?  Injects one fault at a time into a COPY of the scalar oracle (oracle/racc_oracle.c; the SIMD
ports and the wide model stay as they are), builds the copy, and runs tests/test_float_range.py against it through RACC_ORACLE_LIB.
Prints, per fault, the tests that fail.  Nothing in the tree is changed.  CPU only.

    python tools/oracle_fault_injection.py [name-of-one-fault]

DESIGN.md §3 holds the result of the last run."""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAULTS = {
    "select instead of minNum": [("return (a < b || b != b) ? a : b;", "return a < b ? a : b;"), ("return (a > b || b != b) ? a : b;", "return a > b ? a : b;")],
    "T <= |det| tNear turned into <": [("T1 <= absDet1 * tNear", "T1 < absDet1 * tNear"), ("T2 <= absDet2 * tNear", "T2 < absDet2 * tNear")],
    "the pick's > turned into >=": [("T1 * absDet2 > T2 * absDet1", "T1 * absDet2 >= T2 * absDet1")],
    "denormals flushed (FTZ/DAZ around the traversal)": [("    ray_state ray;\n    uint32_t nv = 0, np = 0, maxDepth = 0;",
                                                          "    __builtin_ia32_ldmxcsr(__builtin_ia32_stmxcsr() | 0x8040);\n    ray_state ray;\n    uint32_t nv = 0, np = 0, maxDepth = 0;")],
    "the clamp threshold compared with <=": [("if (fabsf(ray->d[k]) < epsilon)", "if (fabsf(ray->d[k]) <= epsilon)")],
    "maxT = +inf rejected": [("isfinite(ray->tNear) && !isnan(ray->tFar)", "isfinite(ray->tNear) && isfinite(ray->tFar)")],
}


def run(name, edits):
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "oracle")
        shutil.copytree(os.path.join(ROOT, "oracle"), copy, ignore=shutil.ignore_patterns("_ref", "*.so", "__pycache__"))
        path = os.path.join(copy, "racc_oracle.c")
        text = open(path).read()
        for old, new in edits:
            assert old in text, "%s: the oracle no longer reads %r" % (name, old)
            text = text.replace(old, new)
        open(path, "w").write(text)
        subprocess.check_call(["make", "-s", "-C", copy, "libracc_oracle.so"], stdout=subprocess.DEVNULL)
        env = dict(os.environ, RACC_ORACLE_LIB=os.path.join(copy, "libracc_oracle.so"))
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_float_range.py"), "-q", "-p", "no:cacheprovider"],
                             cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True).stdout
        failed = [line.split(" - ")[0][len("FAILED "):] for line in out.splitlines() if line.startswith("FAILED ")]
        print("%s: %s" % (name, "NOT CAUGHT" if not failed else "caught by %d test(s)" % len(failed)))
        for f in failed:
            print("    " + f)
        return bool(failed)


if __name__ == "__main__":
    wanted = sys.argv[1:]
    for fault, edits in FAULTS.items():
        if not wanted or fault in wanted:
            run(fault, edits)
