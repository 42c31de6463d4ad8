"""The surface of aiqmc._lib that code outside it reaches for: every module-level function, class
and constant and every Context attribute not starting with "__", recorded with inspect.signature
before the binding was given one call path (tests/golden/lib_surface.json: names, kinds and
signature strings).  Every recorded name still exists with the recorded signature."""
import inspect
import json
import os

from aiqmc import _lib

# helpers that were only copies of _dev: gone with that change
REMOVED = {"Context._real_dev", "Context._rot"}
# private helpers nothing outside the class calls, whose signature that change set: _dev took over
# the copies' parameters (the old ones still lead, the new ones have defaults), _param_grad names
# the symbol instead of taking the bound function
CHANGED = {
    "Context._dev": "(self, t, n: 'Optional[int]', what: 'Optional[str]' = None, real: 'bool' = False) "
                    "-> 'torch.Tensor'",
    "Context._param_grad": "(self, name: 'str', pos: 'torch.Tensor', weights: 'Optional[torch.Tensor]', "
                           "want_value: 'bool')",
}

# recorded since: the route query of the walker launches (aiqmc_debug_launch_row)
ADDED = {"LAUNCH_KINDS", "Context.launch_row"}


def _recorded(golden_dir):
    with open(os.path.join(golden_dir, "lib_surface.json")) as f:
        return json.load(f)


def _lookup(name):
    obj = _lib
    for part in name.split("."):
        obj = getattr(obj, part)
    return obj


def test_recorded_names_keep_their_signatures(golden_dir):
    rec = _recorded(golden_dir)
    assert len(rec) > 100 and REMOVED | set(CHANGED) | ADDED <= {r["name"] for r in rec}
    missing, moved = [], []
    for r in rec:
        name = r["name"]
        if name in REMOVED:
            assert not hasattr(_lib.Context, name.split(".")[1]), name
            continue
        try:
            obj = _lookup(name)
        except AttributeError:
            missing.append(name)
            continue
        if r["kind"] == "property":
            assert isinstance(obj, property), name
        elif r["kind"] == "class":
            assert inspect.isclass(obj), name
        elif r["kind"] in ("function", "method"):
            want = CHANGED.get(name, r["signature"])
            if str(inspect.signature(obj)) != want:
                moved.append((name, want, str(inspect.signature(obj))))
    assert not missing, missing
    assert not moved, moved


def test_dev_still_binds_the_old_call():
    """_dev's recorded parameters lead the new ones, and what was added has a default."""
    old = ["self", "t", "n"]
    new = list(inspect.signature(_lib.Context._dev).parameters.values())
    assert [p.name for p in new[:len(old)]] == old
    assert all(p.default is not inspect.Parameter.empty for p in new[len(old):])


def test_symbols_and_declarations_agree():
    assert _lib.EXPORTED_SYMBOLS == tuple(_lib._SIGNATURES)
