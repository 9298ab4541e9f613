"""The ctypes prototypes of legged_mpc_control_amd/_native.py against the declarations in include/lmpc/lmpc*.h.

ctypes checks nothing against the library: an argtypes list one short, or a 64-bit return read as an int, corrupts a call
without an error.  So for every function a public header declares, the bound function has as many argtypes as the
declaration has parameters and the restype of its return type; and the names bound are exactly the names declared.
CPU only."""
import ctypes
import glob
import os
import re

import pytest

from conftest import ROOT

from legged_mpc_control_amd import _native as N

RESTYPES = {"void": None, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "const char*": ctypes.c_char_p}
SYMBOLS = {"lmpc.h": N.EXPORTED_SYMBOLS, "lmpc_hoqp.h": N.HOQP_SYMBOLS, "lmpc_rollout.h": N.ROLLOUT_SYMBOLS,
           "lmpc_rbd.h": N.RBD_SYMBOLS, "lmpc_sim.h": N.SIM_SYMBOLS, "lmpc_stack.h": N.STACK_SYMBOLS,
           "lmpc_est.h": N.EST_SYMBOLS, "lmpc_contact.h": N.CONTACT_SYMBOLS, "lmpc_lowlevel.h": N.LOWLEVEL_SYMBOLS,
           "lmpc_lowsim.h": N.LOWSIM_SYMBOLS, "lmpc_multi.h": N.MULTI_SYMBOLS}


def declarations(path):
    """{function: (return type, parameter count)} of a C header."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for ret, name, params in re.findall(r"(?:^|[;}])\s*((?:const\s+)?\w+\s*\**)\s*\b(lmpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src, flags=re.M):
        params = params.strip()
        assert name not in out, name
        out[name] = (re.sub(r"\s+", " ", ret).replace(" *", "*").strip(), 0 if params in ("", "void") else params.count(",") + 1)
    return out


HEADERS = {os.path.basename(p): declarations(p) for p in sorted(glob.glob(os.path.join(ROOT, "include", "lmpc", "lmpc*.h")))}


def test_every_public_header_is_bound_by_name():
    assert sorted(HEADERS) == sorted(SYMBOLS)
    assert sum(len(d) for d in HEADERS.values()) >= 152
    for header, decl in HEADERS.items():
        assert sorted(SYMBOLS[header]) == sorted(decl), header
        assert len(set(SYMBOLS[header])) == len(SYMBOLS[header]), header


@pytest.mark.parametrize("header", sorted(SYMBOLS))
def test_prototypes_match_the_declarations(header):
    if header == "lmpc_multi.h":
        from legged_mpc_control_amd import build as B

        B.build_multi()
        L = N.multi_lib()
    else:
        L = N.lib()
    for name, (ret, nparams) in HEADERS[header].items():
        fn = getattr(L, name)
        assert len(fn.argtypes or ()) == nparams, (name, nparams, fn.argtypes)
        assert ret in RESTYPES, (name, ret)
        assert fn.restype is RESTYPES[ret], (name, ret, fn.restype)


def test_load_errors_name_the_abi_or_the_symbol(tmp_path):
    """A library of another ABI is reported as that and not as the first symbol it lacks; a library of this ABI that
    lacks a symbol is reported with the symbol and its header.  (Two stand-in libraries of one function each.)"""
    import subprocess

    from legged_mpc_control_amd import build as B

    def stub(abi):
        src, out = tmp_path / f"abi{abi}.c", tmp_path / f"libabi{abi}.so"
        src.write_text(f"int lmpc_abi_version(void) {{ return {abi}; }}\n")
        subprocess.run([B.host_cxx(), "-shared", "-fPIC", "-x", "c", "-o", str(out), str(src)], check=True)
        return str(out)

    lmpc_h = [h for h in N._HEADERS if h.name == "lmpc.h"]
    old = stub(N.ABI_VERSION - 1)
    with pytest.raises(N.NativeLibraryError, match=rf"lmpc\.h: the library is ABI {N.ABI_VERSION - 1} .* binding is ABI {N.ABI_VERSION}"):
        N._bind(ctypes.CDLL(old), old, lmpc_h)
    bare = stub(N.ABI_VERSION)
    with pytest.raises(N.NativeLibraryError, match=r"no symbol lmpc_params_go1 \(include/lmpc/lmpc\.h\)"):
        N._bind(ctypes.CDLL(bare), bare, lmpc_h)
