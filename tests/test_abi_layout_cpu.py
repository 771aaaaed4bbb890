"""CPU: every ctypes mirror in efficientlo-net_amd/_lib.py has the size and the field offsets of the struct of the same
name in include/elo.h (a C program compiled against the header prints them).  A drift between the two is silent memory
corruption on the GPU; this catches it where there is no GPU."""
import ctypes
import os
import subprocess

from conftest import ROOT, load_pkg


def test_ctypes_structs_mirror_the_header(tmp_path):
    L = load_pkg("_lib")
    mirrors = {v.__name__: v for v in vars(L).values()
               if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__name__.startswith("elo_")}
    assert len(mirrors) >= 25
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "elo.h"', 'int main(void) {']
    for name, cls in sorted(mirrors.items()):
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in mirrors.items():
        assert ctypes.sizeof(cls) == int(want[name]), name
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == int(want["%s.%s" % (name, field)]), (name, field)


def test_grouping_block_and_its_form_queries():
    """elo_group_args (mirrored as GroupArgs) field by field, and the four form queries that take it: declared in the header,
    bound in the ctypes table with that block as their only argument."""
    import re
    L = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "elo.h")).read()
    body = re.search(r"typedef struct elo_group_args \{(.*?)\} elo_group_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.sub(r"^.*[\s*]", "", name.strip()) for d in body.split(";") if d.strip() for name in d.split(",")]
    assert [name for name, _ in L.GroupArgs._fields_] == declared
    for query in ("elo_fused_conv_random_k_form", "elo_fused_conv_select_k_form", "elo_fused_conv_random_k_dense_form",
                  "elo_fused_conv_select_k_dense_form"):
        assert re.search(r"^int %s\(const elo_group_args \*a\);" % query, header, re.M)
        assert (query, ctypes.c_int, [ctypes.POINTER(L.GroupArgs)]) in L.SYMBOLS
    assert tuple(L.GROUPING_QUERIES) == tuple(q for q in (n for n, _r, _a in L.SYMBOLS) if q.startswith("elo_fused_conv") and q.endswith("_form"))
