"""CPU: the surface of pg_prefill_replicated -- header, export map, ctypes prototype, the share_replicas cfg key -- and the owner rule as a pure
function against a brute-force definition."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT


def test_header_map_and_binding_declare_the_entry_point():
    from plangen_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    m = re.search(r"int\s+pg_prefill_replicated\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/plangen_hip.h does not declare pg_prefill_replicated"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 8 and params[0].startswith("pg_handle") and params[-1].startswith("pg_stream"), params
    assert [p.split()[-1] for p in params[3:7]] == ["R0", "L", "replicas", "alias"], params
    mp = open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    assert re.search(r"\bpg_prefill_replicated;", mp)
    sym = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    res, args = sym["pg_prefill_replicated"]
    assert res is C.c_int and len(args) == 8
    assert args == [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    # selected by the entry point, not by an option: the product's option table does not grow
    api = open(os.path.join(ROOT, "plangen_amd", "csrc", "engine_api.hip")).read()
    opts = api[api.index("int pg_set_option"):api.index("int64_t pg_device_bytes")]
    assert "replica" not in opts


def test_share_replicas_is_an_opt_in_cfg_key():
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    from plangen_amd.system import System
    assert PlanGenConfig().share_replicas == 0 and PlanGenConfig(share_replicas=1).share_replicas == 1
    ns = {}
    exec(open(os.path.join(ROOT, "project", "plangen", "cfg", "base.py")).read(), ns)
    assert ns["share_replicas"] == 0
    assert "share_replicas" in open(os.path.join(ROOT, "project", "plangen", "plangen_base.py")).read()
    sig = inspect.signature(Engine.prefill_replicated).parameters
    assert list(sig)[1:] == ["ids", "pad_len", "replicas", "alias", "uncond_shared"] and sig["alias"].default is True
    # signatures gain keyword arguments only
    si = inspect.signature(System.sample_image).parameters
    assert si["replicas"].default == 1 and list(si)[:5] == ["self", "tokens", "mask", "cfg_weight", "temperature"]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("R0", [2, 4, 6])
def test_owner_rule_against_brute_force(R0, p, shared):
    """owner(row): the first row (in row order) that carries the same prompt AND holds it -- with a shared negative prompt every odd row
    carries row 1's; otherwise row t * R0 + r carries row r's."""
    from plangen_amd.engine import replica_owner
    R = R0 * p
    # prompt identity of every virtual row, by construction of the replicated CFG batch
    ident = [("neg",) if (shared and row % 2 == 1) else ("row", row % R0) for row in range(R)]
    for row in range(R):
        brute = next(q for q in range(R) if ident[q] == ident[row])
        assert replica_owner(row, R0, shared) == brute, (row, R0, p, shared)
        o = replica_owner(row, R0, shared)
        assert o <= row and replica_owner(o, R0, shared) == o            # owners own themselves; aliasing rows come after their owner
    aliasing = [row for row in range(R) if replica_owner(row, R0, shared) != row]
    distinct = len(set(ident))
    assert len(aliasing) == R - distinct                                 # exactly the distinct prompts are prefilled
