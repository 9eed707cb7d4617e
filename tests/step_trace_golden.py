"""tests/golden/step_trace.txt (tools/step_trace.sh; tests/test_step_trace.py holds the tree to it), read back as blocks."""
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_trace.txt")


def golden_blocks(path=GOLDEN):
    """{header of a step: [its trace lines]}: the file numbers every distinct line once and writes a step as the numbers of its lines"""
    text = open(path).read()
    numbered, steps = text.split("== steps", 1)
    lines = {}
    for row in numbered.splitlines()[1:]:
        number, line = re.match(r" *(\d+)(  .*)$", row).groups()
        lines[int(number)] = line
    assert sorted(lines) == list(range(1, len(lines) + 1))
    blocks = {}
    for row in steps.splitlines()[1:]:
        header, seq = row.rsplit(" :", 1)
        assert header not in blocks, header
        blocks[header] = [lines[int(n)] for n in seq.split()]
    return blocks
