"""CPU: the ABI surface of the challenge round's calls (sec_bn_crt_modexp2_batch,
sec_apdp_prove_batch, sec_apdp_verify_batch): declared, exported, additions to ABI version 1, and
SEC_EINVAL for a NULL context before anything else is looked at."""

import os
import re

import numpy as np

from storb_amd import _lib

CALLS = ("sec_bn_crt_modexp2_batch", "sec_apdp_prove_batch", "sec_apdp_verify_batch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_exported():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "storb_ec.h")) as f:
        header = f.read()
    for name in CALLS:
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert lib.sec_abi_version() == 1  # additions: the ABI version stays
    assert "#define SEC_ABI_VERSION 1" in header


def test_argument_counts_match_the_header():
    with open(os.path.join(ROOT, "include", "storb_ec.h")) as f:
        header = f.read()
    for name in CALLS:
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGS[name][1]), name


def test_null_context_is_einval():
    lib = _lib.load()
    z = np.zeros(512, np.uint8)
    p = z.ctypes.data
    msgs = np.zeros(1, dtype=_lib.MSG_DTYPE)
    st = np.zeros(1, np.int32)
    for flags in (0, _lib.SEC_F_HOST):
        assert lib.sec_bn_crt_modexp2_batch(None, None, p, p, p, p, p, p, 1, 1, p, flags) == _lib.SEC_EINVAL
        assert lib.sec_apdp_prove_batch(None, None, msgs.ctypes.data, 1, p, p, p, p, p, p, flags) == _lib.SEC_EINVAL
        assert lib.sec_apdp_verify_batch(None, None, p, p, p, p, p, 1, p, st.ctypes.data, flags) == _lib.SEC_EINVAL
    # a count of zero does not excuse the context
    assert lib.sec_bn_crt_modexp2_batch(None, None, None, None, None, None, None, None, 1, 0, None, 0) == _lib.SEC_EINVAL
    assert lib.sec_apdp_prove_batch(None, None, None, 0, None, None, None, None, None, None, 0) == _lib.SEC_EINVAL
    assert lib.sec_apdp_verify_batch(None, None, None, None, None, None, None, 0, None, None,
                                     _lib.SEC_F_HOST) == _lib.SEC_EINVAL
