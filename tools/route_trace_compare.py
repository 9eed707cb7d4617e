"""Compares two outputs of tools/route_trace.sh: `python tools/route_trace_compare.py a.txt b.txt`.  A record's launcher is reduced to its
name and template arguments (the parameter list goes, and the dispatch functions' own names are mapped onto one another), so a launch site
that moved to another function still compares on kernel expression, template arguments, dimensions and argument hash.  Exit status 1 and the
first differing records when the two trees route differently."""
import gzip
import re
import sys

PARAMS = re.compile(r"\| (?:static )?hipError_t sdqn::(\w+)\([^|\[]*\)")
RENAMED = {"launch_kernel_ss": "launch_ss", "launch_kernel_bt": "launch_bt", "launch_kernel_r3": "launch_r3", "launch_kernel_ext": "launch_ext",
           "launch_kernel_h16": "launch_ext", "launch_kernel": "launch_lat"}


def records(path):
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        for line in f:
            yield PARAMS.sub(lambda m: "| " + RENAMED.get(m.group(1), m.group(1)), line.rstrip("\n"))


if __name__ == "__main__":
    n = bad = 0
    a, b = records(sys.argv[1]), records(sys.argv[2])
    for ra in a:
        rb = next(b, None)
        n += 1
        if ra != rb:
            bad += 1
            if bad <= 20:
                print("- %s\n+ %s" % (ra, rb))
    extra = sum(1 for _ in b)
    print("%d records compared, %d differ, %d only in the second file: %s" % (n, bad, extra, "identical" if not bad and not extra else "DIFFERENT"))
    sys.exit(1 if bad or extra else 0)
