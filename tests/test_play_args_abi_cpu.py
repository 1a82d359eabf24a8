"""rvz_play_args across the C header and its ctypes mirror (rvz._lib.PlayArgs): every field at the
header's offset, the same size, and the fields added for the forced searches
(skip_forced_roots, roots_unread) appended after rows_unread, so that a caller
built against the earlier struct and zero-filling it gets the earlier behaviour."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_layout(tmp_path, fields):
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler (the oracle's build needs one too)"
    src = tmp_path / "layout.c"
    lines = "".join(f'    printf("{f} %zu\\n", offsetof(rvz_play_args, {f}));\n' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rvz.h"\n'
                   'int main(void) {\n' + lines +
                   '    printf("sizeof %zu\\n", sizeof(rvz_play_args));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def test_play_args_mirror_matches_the_header(tmp_path):
    from rvz._lib import PlayArgs
    names = [f[0] for f in PlayArgs._fields_]
    layout = _header_layout(tmp_path, names)
    assert layout.pop("sizeof") == C.sizeof(PlayArgs)
    for n in names:
        assert layout[n] == getattr(PlayArgs, n).offset, n
    # appended: the last two fields, after everything the earlier struct held
    assert names[-3:] == ["rows_unread", "skip_forced_roots", "roots_unread"]
    assert sorted(layout, key=layout.get)[-2:] == ["skip_forced_roots", "roots_unread"]
    end = PlayArgs.roots_unread.offset + PlayArgs.roots_unread.size
    assert end == C.sizeof(PlayArgs)
    assert PlayArgs.skip_forced_roots.offset >= PlayArgs.rows_unread.offset + 8


def test_play_args_defaults_leave_the_switch_off():
    from rvz._lib import PlayArgs
    a = PlayArgs()
    assert a.skip_forced_roots == 0 and not a.roots_unread
