"""Writes tests/golden/jpeg_front_pins.json: per case of tests/jpeg_front_cases.py a digest of everything the JPEG host front ends return for it.

The pins are the verdicts of the commit BEFORE the front ends were given one marker walk, and are made there: in a checkout of
that commit, built, with this file and tests/jpeg_front_cases.py copied in,

    python tests/golden/make_jpeg_front_pins.py

Both files go through capi.lib() and entry points that commit has already, so they run there unmodified.  --check compares instead of writing."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_front_cases as FC  # noqa: E402
from ffpic_amd import capi  # noqa: E402

PATH = os.path.join(HERE, "jpeg_front_pins.json")


def text():
    L = capi.lib()
    rows = [json.dumps([tag, *FC.verdict(L, data)]) for tag, data in FC.cases()]
    return '{"cases": [\n' + ",\n".join(rows) + "\n]}\n"


if __name__ == "__main__":
    new = text()
    if "--check" in sys.argv[1:]:
        sys.exit(0 if open(PATH).read() == new else "jpeg_front_pins.json differs from what this library gives")
    open(PATH, "w").write(new)
    print(f"{PATH}: {new.count(chr(10)) - 2} cases")
