"""What the six ctypes bindings inherit from ccnet_amd/_clib.py, checked once per binding without a GPU: a missing library and
a library of another ABI version are refused with that binding's own error."""
import importlib

import pytest

BINDINGS = [("_lib", "CcaLibrary", "CcaError", "CCNET_CCA_VERSION"),
            ("_ohem_lib", "OhemLibrary", "OhemError", "CCNET_OHEM_VERSION"),
            ("_eval_lib", "EvalLibrary", "EvalError", "CCNET_EVAL_VERSION"),
            ("_lovasz_lib", "LovaszLibrary", "LovaszError", "CCNET_LOVASZ_VERSION"),
            ("_abn_lib", "AbnLibrary", "AbnError", "CCNET_ABN_VERSION"),
            ("_proj_lib", "ProjLibrary", "ProjError", "CCNET_PROJ_VERSION")]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()                      # hipcc cross-compiles gfx950 without a GPU


@pytest.mark.parametrize("module,library,error,version", BINDINGS, ids=[b[0] for b in BINDINGS])
def test_binding_refuses_a_missing_library_and_another_abi_version(built, module, library, error, version, tmp_path, monkeypatch):
    m = importlib.import_module("ccnet_amd." + module)
    Library, Error = getattr(m, library), getattr(m, error)
    others = [getattr(importlib.import_module("ccnet_amd." + b[0]), b[2]) for b in BINDINGS if b[0] != module]
    assert issubclass(Error, RuntimeError) and not any(issubclass(Error, o) or issubclass(o, Error) for o in others)
    with pytest.raises(Error, match="not found"):
        Library(str(tmp_path / "libccnet_missing.so"))
    assert Library(m.LIB_PATH).path == m.LIB_PATH           # loads as built
    monkeypatch.setattr(m, version, getattr(m, version) + 1)
    with pytest.raises(Error, match="rebuild"):
        Library(m.LIB_PATH)
