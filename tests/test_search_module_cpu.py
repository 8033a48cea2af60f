"""Where the search API lives: ewn_gym_amd.search holds the calls on a trained network, ewn_gym_amd._args what every binding needs,
and ewn_gym_amd.vec_env still offers every name it used to.  No GPU is needed: nothing here launches."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEARCH_NAMES = ["predict_policy", "predict_lookahead", "lookahead_expand", "lookahead_reduce", "lookahead_targets", "sup_grad", "predict_puct",
                "puct_begin", "puct_advance", "puct_result", "puct_tree_views", "puct_play", "selfplay_noise", "selfplay_outcomes",
                "selfplay_puct", "puct_search"]

# One fresh interpreter imports each module alone and first, every time with nothing of the package loaded.  The package's __init__
# imports every module, so "what does this module import" is asked with a bare package in its place; then each import is repeated
# with the package as it is.
SCRIPT = """
import importlib, sys, types
def forget():
    for m in [m for m in sys.modules if m.split('.')[0] == 'ewn_gym_amd']:
        del sys.modules[m]
for module in ('_args', 'endgame', 'search'):
    forget()
    pkg = types.ModuleType('ewn_gym_amd')
    pkg.__path__ = [%r]
    sys.modules['ewn_gym_amd'] = pkg
    importlib.import_module('ewn_gym_amd.' + module)
    print(module, *sorted(m for m in sys.modules if m.startswith('ewn_gym_amd.')))
    forget()
    importlib.import_module('ewn_gym_amd.' + module)
    print(module, sys.modules['ewn_gym_amd'].__all__[0])
""" % os.path.join(ROOT, "ewn_gym_amd")


def test_the_search_names_are_one_object_in_the_package_in_search_and_in_vec_env():
    pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd import search, vec_env
    assert sorted(SEARCH_NAMES) == sorted(n for n in ewn_gym_amd.__all__ if getattr(getattr(ewn_gym_amd, n), "__module__", None) == search.__name__)
    for name in SEARCH_NAMES:
        assert getattr(ewn_gym_amd, name) is getattr(search, name) is getattr(vec_env, name), name
    for name in ("_ptr", "_stream", "_puct_sections", "_puct_search", "PUCT_LAYOUT", "SELFPLAY_MAX_PLIES", "LA_ROWS"):   # what tests and tools take
        assert hasattr(vec_env, name), name


def test_each_module_imports_alone_and_first_and_args_needs_no_sibling_but_lib():
    pytest.importorskip("torch")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [
        "_args ewn_gym_amd._args ewn_gym_amd._lib", "_args VecEWN",
        "endgame ewn_gym_amd._args ewn_gym_amd._lib ewn_gym_amd.endgame", "endgame VecEWN",      # no way round through vec_env
        "search ewn_gym_amd._args ewn_gym_amd._lib ewn_gym_amd.endgame ewn_gym_amd.search", "search VecEWN"]
