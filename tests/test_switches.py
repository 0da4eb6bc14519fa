"""The engine's FFM_* environment switches (grid sizes, workgroup sizes, LDS parking, range order,
stream use) are scheduling choices: every one must give the oracle's bits.  Two rules keep that
testable, checked here over the HIP sources without a GPU -- as a lint: the static check looks at
the statement that holds the getenv call, so it does not see a switch read in the default member
initializer of a namespace-scope object (how FFM_HOST_TIMING is read; exempt below) or one read
through a helper whose result is cached elsewhere:

- every switch is read when an engine is created, never held in `static` storage: a value cached on
  the first call of a process would make a test that sets the switch later run the cached value;
- every switch the engine reads is named by at least one test module, so that a new switch comes
  with a test (tools/ scripts do not count: they are not part of the suite).
"""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ftrl-ffm_amd", "csrc")

# switches exempt from both rules, with the reason
EXEMPT = {
    "FFM_HOST_TIMING": "process-wide debug printout of host wall time, summed over every engine and "
                       "printed at exit; it changes no launch",
}

GETENV = re.compile(r'getenv\(\s*"(FFM_\w+)"\s*\)')


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")))
    assert paths, "no HIP sources under " + CSRC
    out = {}
    for p in paths:
        with open(p) as f:
            out[os.path.basename(p)] = f.read()
    return out


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _statement(code, pos):
    """The C++ statement around position `pos`: from after the previous ';', '{' or '}' up to the
    next ';'."""
    lo = max(code.rfind(c, 0, pos) for c in ";{}") + 1
    hi = code.find(";", pos)
    return code[lo:hi if hi >= 0 else len(code)]


def _switches():
    """{name: [(file, line, statement)]} of every getenv("FFM_...") in the sources."""
    found = {}
    for name, text in _sources().items():
        code = _strip_comments(text)
        for m in GETENV.finditer(code):
            line = code.count("\n", 0, m.start()) + 1
            found.setdefault(m.group(1), []).append((name, line, _statement(code, m.start())))
    return found


def test_the_sources_read_switches():
    found = _switches()
    # (the scan itself: the switches the update grids and the row kernel's parking are set by)
    for name in ("FFM_GRID_HOT", "FFM_GRID_GIANT", "FFM_ROW_PARK", "FFM_ROW_PARK_BUDGET", "FFM_UPDATE_ORDER"):
        assert name in found, name
    assert set(EXEMPT) <= set(found), "an exempt switch no longer exists: drop it from EXEMPT"


def test_no_switch_is_held_in_static_storage():
    bad = []
    for name, sites in sorted(_switches().items()):
        if name in EXEMPT:
            continue
        for fname, line, stmt in sites:
            if re.search(r"\bstatic\b", stmt) or re.search(r"\bthread_local\b", stmt):
                bad.append("%s:%d %s" % (fname, line, name))
    assert not bad, ("switches held in static storage (read once per process, so an engine created "
                     "after the switch changes ignores it): " + ", ".join(bad))


def test_the_static_check_sees_a_function_local_static():
    code = 'int f() {\n  if (x) {\n    static const int v = std::getenv("FFM_X") ? 1 : 0;\n  }\n}\n'
    m = GETENV.search(code)
    assert re.search(r"\bstatic\b", _statement(code, m.start()))
    code = 'void g(E *e) { if (const char *sv = std::getenv("FFM_X")) e->x = 1; }'
    m = GETENV.search(code)
    assert not re.search(r"\bstatic\b", _statement(code, m.start()))


def test_every_switch_is_named_by_a_test():
    tests = ""
    for p in sorted(glob.glob(os.path.join(HERE, "test_*.py"))):
        if os.path.basename(p) == os.path.basename(__file__):
            continue  # (naming a switch here is not testing it)
        with open(p) as f:
            tests += f.read() + "\n"
    missing = [name for name in sorted(_switches()) if name not in EXEMPT
               and not re.search(r"\b%s\b" % re.escape(name), tests)]
    assert not missing, "switches no test module names: " + ", ".join(missing)
