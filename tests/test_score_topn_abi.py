"""CPU: the prompt top-N entries (include/bitnet_hip_scoretopn.h): the refusals added to bitnet_hip_score_f16_dev's, before anything launches, and
the workspace size: the score workspace plus 4 keys, 4 ids and a certificate per (padded row, 128-entry block), no [n, vocab] term."""
import ctypes as C
import os

import pytest

FAKE = 4096  # a non-null "device pointer": every refusal below happens before anything is dereferenced


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load()


def test_entries_are_declared_exported_and_spelt_out_for_rust(pkg, lib):
    names = {name for name, _, _ in pkg.scoretopn_prototypes()}
    assert names == {"bitnet_hip_score_topn_workspace_bytes", "bitnet_hip_score_topn_f16_dev"} <= set(pkg.declared_symbols())
    assert all(hasattr(lib.c, n) for n in names) and hasattr(C.CDLL(pkg.HOST_LIB_PATH), "bitnet_host_score_topn")
    text = open(os.path.join(os.path.dirname(pkg.HEADER_PATH), os.pardir, "INTEGRATION.md")).read()
    assert all(f"pub fn {n}(" in text for n in names) and '#include "bitnet_hip_scoretopn.h"' in open(pkg.HEADER_PATH).read()


def call(lib, **kw):
    a = dict(table=FAKE, x=FAKE, gamma=FAKE, eps=1e-5, hidden=512, vocab=1000, n_rows=4, targets=FAKE, nll=FAKE, argmax=None, records=FAKE,
             top_n=5, workspace=FAKE, workspace_bytes=1 << 40)
    a.update(kw)
    lib.score_topn_f16_dev(a.pop("table"), a.pop("x"), a.pop("gamma"), a.pop("eps"), a.pop("hidden"), a.pop("vocab"), a.pop("n_rows"),
                           a.pop("targets"), a.pop("nll"), **a)


@pytest.mark.parametrize("kw,msg", [
    (dict(records=None), "Null pointer"),
    (dict(top_n=0), "top_n must be in 1..20, got 0"),
    (dict(top_n=21), "top_n must be in 1..20, got 21"),
    (dict(hidden=100), "multiple of 64"),
    (dict(workspace_bytes=1000), "workspace too small: 184832 bytes needed, 1000 given"),
])
def test_refusals_before_device_work(pkg, lib, kw, msg):
    with pytest.raises(pkg.BitNetHipError, match=msg) as e:
        call(lib, **kw)
    assert e.value.code == pkg.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("n,h,v,n_pad,blocks", [(4096, 2560, 128256, 4096, 1002), (1, 512, 1000, 128, 8), (0, 512, 1000, 0, 0), (1, 512, 0, 0, 0),
                                                (1 << 62, 2560, 128256, 0, 0)])
def test_workspace_is_the_score_workspace_plus_candidates_and_certificates_and_zero_where_that_is(lib, n, h, v, n_pad, blocks):
    assert (lib.score_workspace_bytes(n, h, v) == 0) == (n_pad == 0)
    assert lib.score_topn_workspace_bytes(n, h, v) == lib.score_workspace_bytes(n, h, v) + n_pad * blocks * (4 * 8 + 4)
