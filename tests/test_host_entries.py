"""CPU test of the C-ABI across the host translation units (vr_capi.hip holds the entries, the other host
files what they call): every function declared in include/vrhip.h resolves by its plain C name."""
import ctypes
import os
import re

from volume_renderer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_entry_resolves_as_a_c_symbol():
    """Each function name of include/vrhip.h (comments of both kinds stripped) is looked up through ctypes
    in the loaded library -- an entry that lost its extern "C" would only exist under a mangled name."""
    src = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    names = sorted(set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src)))
    assert len(names) >= 50 and "vr_new" in names and "vr_version" in names, names  # (54 entries today)
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = []
    for n in names:
        try:
            getattr(L, n)
        except AttributeError:
            missing.append(n)
    assert not missing, missing
