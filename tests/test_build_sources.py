"""The build script's source list against the directory it compiles (no GPU, no build): a forgotten or misspelt entry of
matcouply_amd/_build.py fails here by name instead of as an undefined symbol when the library is linked."""
import collections
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_module():
    # by path: importing the package would pull in torch, and nothing here needs it
    spec = importlib.util.spec_from_file_location("_mcl_build_script", os.path.join(REPO, "matcouply_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sources_list_every_hip_file_once():
    build = _build_module()
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert on_disk, build.CSRC
    counts = collections.Counter(build.SOURCES)
    assert [f for f, n in counts.items() if n > 1] == [], "listed more than once"
    assert sorted(set(on_disk) - set(counts)) == [], "in csrc/ but not in SOURCES: never compiled"
    assert sorted(set(counts) - set(on_disk)) == [], "in SOURCES but not in csrc/"


def test_extra_flags_name_listed_sources():
    build = _build_module()
    assert sorted(set(build.EXTRA_FLAGS) - set(build.SOURCES)) == [], "EXTRA_FLAGS entry for a file that is not compiled"
