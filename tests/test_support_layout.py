"""Where shared test code lives: in support modules under tests/ (no `test_` in their names, no test functions in them), never
in a test module that another test module or a tool imports.  Reads the files as text; no GPU, nothing of the project imported."""
import glob
import os
import re

TESTS = os.path.dirname(os.path.abspath(__file__))
SUPPORT = ("pairs_device", "pairs_cases", "eval_support", "lm_support", "pairs_api_support", "pairs_depth_support", "stream_backlog", "pairs_track_support")
IMPORTS_A_TEST_MODULE = re.compile(r"^\s*(from|import)\s+test_\w+", re.M)
DEFINES_A_TEST = re.compile(r"^\s*def\s+test\w*", re.M)


def test_no_test_module_or_tool_imports_a_test_module():
    paths = sorted(glob.glob(os.path.join(TESTS, "*.py")) + glob.glob(os.path.join(os.path.dirname(TESTS), "tools", "*.py")))
    assert len(paths) > 50
    bad = [(os.path.relpath(p, TESTS), m.group(0).strip()) for p in paths for m in IMPORTS_A_TEST_MODULE.finditer(open(p).read())]
    assert not bad, bad


def test_support_modules_exist_and_define_no_tests():
    for name in SUPPORT:
        path = os.path.join(TESTS, name + ".py")
        assert os.path.isfile(path), name
        assert not DEFINES_A_TEST.search(open(path).read()), name
