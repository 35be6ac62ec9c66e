"""CPU: every run-time option (bis_set_option / BIS_* variables) is declared once, read by the library, and named by a test.

The options table (BIS_OPTIONS_ENV / BIS_OPTIONS_API in bis_blas1.hip) and the fields of struct bis_options
(bis_internal.hpp) must be the same set; every option must be read somewhere as `bis_opts().<name>` outside the table
machinery (an option nobody reads describes a run that did not happen); and every option must be named in some test
module other than this one -- as a quoted string or as its BIS_<NAME> variable -- or carry a stated reason in EXEMPT.
An option added later without a test fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basic_iterative_solvers_amd", "csrc")

EXEMPT = {
    "trsv_tile_exp": "timing experiments only: its results are wrong by design, and it is refused unless the library is "
                     "built with -DBIS_TILED_EXP",
}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def table_options():
    text = _strip_comments(open(os.path.join(CSRC, "bis_blas1.hip")).read())
    tables = {}
    for macro, arg in (("BIS_OPTIONS_ENV", "X"), ("BIS_OPTIONS_API", "Y")):
        m = re.search(r"#define\s+%s\(%s\)([^\n]*)" % (macro, arg), text)
        assert m, f"{macro} not found"
        tables[macro] = re.findall(r"\b%s\((\w+)\)" % arg, m.group(1))
    return tables


def struct_fields():
    text = _strip_comments(open(os.path.join(CSRC, "bis_internal.hpp")).read())
    m = re.search(r"struct\s+bis_options\s*\{(.*?)\n\};", text, flags=re.S)
    assert m, "struct bis_options not found"
    return re.findall(r"\bint\s+(\w+)\s*=\s*-1\s*;", m.group(1))


def all_options():
    t = table_options()
    return t["BIS_OPTIONS_ENV"] + t["BIS_OPTIONS_API"]


def test_tables_and_struct_are_the_same_set():
    t = table_options()
    env, api = t["BIS_OPTIONS_ENV"], t["BIS_OPTIONS_API"]
    fields = struct_fields()
    assert len(env) + len(api) >= 40 and len(fields) >= 40
    dup = sorted({o for o in env + api if (env + api).count(o) > 1})
    assert not dup, f"options listed twice: {dup}"
    assert len(set(fields)) == len(fields)
    assert sorted(env + api) == sorted(fields), (sorted(set(env + api) - set(fields)), sorted(set(fields) - set(env + api)))


def test_every_option_is_read_by_the_library():
    reads = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        text = _strip_comments(open(path).read())
        reads |= set(re.findall(r"\bbis_opts\(\)\s*\.\s*(\w+)", text))
    unread = [o for o in all_options() if o not in reads]
    assert not unread, f"options declared and settable but never read (bis_opts().<name>): {unread}"


def test_every_option_is_named_by_a_test():
    me = os.path.abspath(__file__)
    texts = [open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) if os.path.abspath(p) != me]
    blob = "\n".join(texts)
    for name, reason in EXEMPT.items():
        assert name in all_options(), f"EXEMPT names an option that does not exist: {name}"
        assert len(reason.split()) >= 5, f"EXEMPT entry {name} needs a stated reason"
    untested = [o for o in all_options() if o not in EXEMPT and not re.search(
        r"[\"']%s[\"']|\bBIS_%s\b|\b%s=" % (o, o.upper(), o), blob)]
    assert not untested, f"options no test sets (name one in a test, or give a reason in EXEMPT): {untested}"
