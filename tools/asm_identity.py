#!/usr/bin/env python3
"""Device assembly of the three objects built from pmpc_ipm.hip, function by function, old against new.

    tools/asm_identity.py OLD NEW [--jobs N] [--keep DIR]

OLD and NEW are each a source tree (its csrc/Makefile gives the compile line of every object: main,
-DPMPC_SEQ and -DDART_WG=2) or a directory that already holds the device assembly as ipm.s, seq.s and
wg2.s (what --keep DIR leaves behind, DIR/old and DIR/new).  Needs hipcc; no GPU.

One line per function: object, instructions in OLD, `identical` or `DIFFERENT (n -> m instructions)`, the
demangled name.  Only instruction text is compared, with comments, labels and directives removed.  Functions
are matched by demangled name; a function without a name match is matched to an unmatched old function of the
same object with the same instruction text (a rename), failing that to the most similar one left, and reported
as such.  Where functions are both renamed and changed, --renames takes the pairs from the report of the change
that only renamed them.  Exit status 1 if anything differs.

--object KEY=TARGET (repeatable) compares other objects of the Makefile instead, e.g. --object loop=build/loop_step.o
for the closed-loop glue kernels of loop_step.hip.

--resources prints, for the same pairs, the compiler's own figures from the assembly's summary comments (VGPRs, AGPRs,
scratch and LDS bytes, the occupancy compiled for), old -> new.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("dart-dual-arm-non-prehensile-manipulation_amd", "csrc")
OBJECTS = {"ipm": "build/pmpc_ipm.o", "seq": "build/pmpc_seq.o", "wg2": "build/pmpc_wg2.o"}


def compile_lines(tree):
    """The Makefile's own hipcc line of each object (make -n), turned into a device-assembly line."""
    csrc = os.path.join(tree, CSRC)
    out = subprocess.run(["make", "-n", "-B"] + list(OBJECTS.values()), cwd=csrc, check=True, capture_output=True,
                         text=True).stdout
    lines = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv or "-o" not in argv:
            continue
        target = argv[argv.index("-o") + 1]
        for key, obj in OBJECTS.items():
            if target == obj:
                i = argv.index("-o")
                lines[key] = [a for j, a in enumerate(argv) if a != "-c" and j not in (i, i + 1)]
    missing = set(OBJECTS) - set(lines)
    if missing:
        sys.exit("%s: no compile line for %s" % (csrc, ", ".join(sorted(missing))))
    return csrc, lines


def assemble(tree, dest, jobs):
    """dest/{ipm,seq,wg2}.s from a source tree; a directory that already holds them is used as it is."""
    if all(os.path.isfile(os.path.join(tree, k + ".s")) for k in OBJECTS):
        return tree
    os.makedirs(dest, exist_ok=True)
    csrc, lines = compile_lines(tree)

    def one(key):
        cmd = lines[key] + ["-S", "--cuda-device-only", "-o", os.path.abspath(os.path.join(dest, key + ".s"))]
        if subprocess.run(cmd, cwd=csrc).returncode:
            sys.exit("%s: %s.s did not compile" % (tree, key))

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, OBJECTS))
    return dest


def functions(path):
    """{mangled name: [instruction text]} of one assembly file."""
    out, name, want = {}, None, set()
    for raw in open(path):
        line = raw.split(";", 1)[0].strip()
        m = re.match(r"\.type\s+([^,\s]+),@function", line)
        if m:
            want.add(m.group(1))
            continue
        if line.endswith(":") and " " not in line:
            label = line[:-1]
            if label in want:
                name = label
                out[name] = []
            elif label.startswith(".Lfunc_end"):
                name = None
            continue
        if not line or line.startswith(".") or name is None:
            continue
        # block labels carry the function's index in the file, which a renamed kernel changes
        out[name].append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split())))
    return out


def resources(path):
    """{mangled name: {field: value}} from the compiler's summary comment after each function."""
    out, name, want = {}, None, set()
    for raw in open(path):
        line = raw.strip()
        m = re.match(r"\.type\s+([^,\s]+),@function", line)
        if m:
            want.add(m.group(1))
        elif line.split(";", 1)[0].strip()[:-1] in want:
            name = line.split(";", 1)[0].strip()[:-1]
            out[name] = {}
        m = re.match(r"; (NumVgprs|NumAgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", line)
        if m and name:
            out[name].setdefault(m.group(1), int(m.group(2)))
    return out


def resource_table(old_dir, new_dir, out):
    """VGPRs, AGPRs, scratch and LDS bytes and the occupancy (waves per SIMD) each function is compiled for, old -> new."""
    fields = ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")
    out.write("# object, " + ", ".join("%s old -> new" % f for f in fields) + ", function (new name)\n")
    for key in OBJECTS:
        old_f, new_f = functions(os.path.join(old_dir, key + ".s")), functions(os.path.join(new_dir, key + ".s"))
        old_r, new_r = resources(os.path.join(old_dir, key + ".s")), resources(os.path.join(new_dir, key + ".s"))
        dm = demangle(sorted(set(old_f) | set(new_f)))
        back = {dm[k]: k for k in list(old_f) + list(new_f)}
        pairs = match({dm[k]: v for k, v in old_f.items()}, {dm[k]: v for k, v in new_f.items()})[0]
        for name in sorted(pairs):
            o, n = old_r[back[pairs[name]]], new_r[back[name]]
            cells = " ".join("%5s -> %-5s" % (o.get(f, "-"), n.get(f, "-")) for f in fields)
            out.write("%-5s %s  %s%s\n" % (key, cells, "" if all(o.get(f) == n.get(f) for f in fields) else "CHANGED ",
                                         name[:160]))


def demangle(names):
    if not names:
        return {}
    filt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt")
    res = subprocess.run([filt if os.path.exists(filt) else "c++filt"], input="\n".join(names) + "\n", check=True,
                         capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, res))


def closest(spare, text):
    """The old function left over whose instruction text is most like `text` (a renamed function that changed)."""
    def ratio(k):
        return difflib.SequenceMatcher(None, spare[k], text, autojunk=False).quick_ratio()
    return max(sorted(spare), key=ratio, default=None)


RENAMES = {}      # new name -> old name, from an earlier report (--renames)


def match(old, new):
    """({new name: old name}, {old name: text} left over): by name, by an earlier report's renames, then renamed with
    equal text, then renamed and closest."""
    pairs = {name: name for name in new if name in old}
    pairs.update({name: RENAMES[name] for name in new if name not in old and RENAMES.get(name) in old})
    spare = {k: v for k, v in old.items() if k not in pairs.values()}
    for exact in (True, False):
        for name in sorted(new):
            if name in pairs:
                continue
            twin = (next((k for k in sorted(spare) if spare[k] == new[name]), None) if exact
                    else closest(spare, new[name]))
            if twin is not None:
                pairs[name] = twin
                del spare[twin]
    return pairs, spare


def compare(old_dir, new_dir, out):
    differs = False
    for key in OBJECTS:
        old, new = functions(os.path.join(old_dir, key + ".s")), functions(os.path.join(new_dir, key + ".s"))
        dm = demangle(sorted(set(old) | set(new)))
        old = {dm[k]: v for k, v in old.items()}
        new = {dm[k]: v for k, v in new.items()}
        pairs, spare = match(old, new)
        for name in sorted(new):
            twin = pairs.get(name)
            if twin is None:
                out.write("%-5s %6s %-50s %s\n" % (key, "-", "NEW (%d instructions)" % len(new[name]), name[:160]))
                differs = True
                continue
            was, shown = old[twin], name if twin == name else "%s  (was %s)" % (name, twin)
            if was == new[name]:
                verdict = "identical"
            else:
                verdict = "DIFFERENT (%d -> %d instructions)" % (len(was), len(new[name]))
                differs = True
            out.write("%-5s %6d %-50s %s\n" % (key, len(was), verdict, shown[:260]))
        for name in sorted(spare):
            out.write("%-5s %6d %-50s %s\n" % (key, len(spare[name]), "GONE", name[:160]))
            differs = True
    return differs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=3)
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly under DIR/old and DIR/new")
    ap.add_argument("--renames", metavar="REPORT", help="an earlier report of this tool: its `NEW  (was OLD)` pairs "
                    "name the renamed functions (a names-only change's report, for a later change that alters them)")
    ap.add_argument("--resources", action="store_true", help="print the register / scratch / LDS table instead")
    ap.add_argument("--object", action="append", metavar="KEY=TARGET", help="compare these objects of csrc/Makefile "
                    "(KEY.s from the compile line of TARGET) instead of the three built from pmpc_ipm.hip")
    a = ap.parse_args()
    if a.object:
        OBJECTS.clear()
        OBJECTS.update(dict(o.split("=", 1) for o in a.object))
    if a.renames:
        for line in open(a.renames):
            m = re.search(r"((?:void |bool )?\S+::\S.*?)  \(was (.*)\)$", line.rstrip())
            if m:
                RENAMES[m.group(1)] = m.group(2)
    with tempfile.TemporaryDirectory() as tmp:
        base = a.keep or tmp
        old_dir = assemble(a.old, os.path.join(base, "old"), a.jobs)
        new_dir = assemble(a.new, os.path.join(base, "new"), a.jobs)
        if a.resources:
            resource_table(old_dir, new_dir, sys.stdout)
            return 0
        what = ("the three objects built from pmpc_ipm.hip (main, -DPMPC_SEQ, -DDART_WG=2)" if not a.object
                else ", ".join(OBJECTS.values()))
        print("# device assembly of %s, function by "
              "function,\n# old against new: instruction text with comments, labels and directives removed\n"
              "# object, instructions in the old build, result, function" % what)
        return 1 if compare(old_dir, new_dir, sys.stdout) else 0


if __name__ == "__main__":
    sys.exit(main())
