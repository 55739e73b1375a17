#!/usr/bin/env python3
"""INTEGRATION.md section 1 -- the replacement body of CLZMatcher::do_matching -- as a compilable C++ file.

TEST INFRASTRUCTURE ONLY.  `make -C oracle ref` compiles its output against the reference's own headers into
oracle/_ref/integration_stub.o (tools/check_integration_stub.sh does the same check by hand); the test-suite checks
that object against the current INTEGRATION.md.  Usage: integration_stub.py INTEGRATION.md OUT.cpp
"""
import re
import sys


def stub_source(md_path):
    """The first ```cpp block of section 1, behind the includes it needs."""
    with open(md_path) as f:
        md = f.read()
    sec = md[md.index("## 1. The stub"):]
    code = re.search(r"```cpp\n(.*?)```", sec, re.S).group(1)
    return '#include <algorithm>\n#include <iostream>\n#include <vector>\n#include "lz_matcher.h"\n' + code


if __name__ == "__main__":
    with open(sys.argv[2], "w") as f:
        f.write(stub_source(sys.argv[1]))
