"""Texts for the text-parser tests (tests/test_text_parse_host.py, tests/test_gpu_text_parse.py): texts made of the
device grammar only (csrc/text_parse.h "Text blocks"), and single lines outside it."""
import numpy as np

from ftrl_ffm_amd import synth


def _entry(has_field, f, i, v):
    return ("%d:%d:%s" % (f, i, v)) if has_field else ("%d:%s" % (i, v))


def random_values(n, seed):
    """n spellings of [-]digits[.digits] with at most 7 significant and 10 fraction digits: leading zeros, "1." and
    ".5" forms included."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        n_frac = int(rng.integers(0, 11))
        s = int(rng.integers(1, 8))
        d = str(int(rng.integers(10 ** (s - 1), 10 ** s)))
        d = d.rjust(n_frac + 1, "0") if rng.random() < 0.8 else d.rjust(n_frac, "0")
        whole, frac = (d[:len(d) - n_frac], d[len(d) - n_frac:]) if n_frac else (d, "")
        if whole and rng.random() < 0.1:
            whole = "0" * int(rng.integers(1, 4)) + whole
        if n_frac == 0:
            text = whole + ("." if rng.random() < 0.1 else "")
        else:
            text = whole + "." + frac
        if text in (".", ""):
            text = "0"
        out.append(("-" if rng.random() < 0.3 else "") + text)
    return out


def fast_texts(has_field):
    """name -> bytes, each inside the grammar."""
    E = lambda f, i, v: _entry(has_field, f, i, v)  # noqa: E731
    t = {}
    g = synth.Generator(8, 10000, "zipf", seed=7)
    t["synth"] = synth.to_libffm_text(g.block(300), libsvm=not has_field)
    g39 = synth.Generator(39, 39 * 4000, "zipf", seed=8)
    t["synth39"] = synth.to_libffm_text(g39.block(200), libsvm=not has_field)
    vals = random_values(20000, 11)
    rng = np.random.default_rng(12)
    lines = []
    for r in range(0, len(vals), 10):
        lines.append("1 " + " ".join(E(int(rng.integers(0, 40)), int(rng.integers(0, 10 ** 9)), v) for v in vals[r:r + 10]))
    t["values"] = "\n".join(lines) + "\n"
    t["blanks"] = "  1   %s  %s   \n 0 %s\n   \n1    %s  \n" % (E(0, 1, "1"), E(1, 2, "0.5"), E(2, 3, "2"), E(3, 4, "1"))
    t["crlf"] = "1 %s %s\r\n0 %s\r\n\r\n1\r\n" % (E(0, 1, "1"), E(1, 2, "0.25"), E(2, 3, "1"))
    t["no_final_newline"] = "1 %s\n0 %s %s" % (E(0, 1, "1"), E(1, 2, "3"), E(2, 5, "0.125"))
    t["blank_lines"] = "\n\n1 %s\n\n\r\n   \n \r\n0 %s\n\n" % (E(0, 1, "1"), E(1, 2, "1"))
    t["label_only"] = "1\n0\n-1\n+1\n2\n 1 \n"
    t["labels"] = "".join("%s %s\n" % (lab, E(0, 7, "1")) for lab in ("1", "0", "-1", "+1", "2", "-0", "+0", "007", "123456789"))
    t["zeros"] = "1 %s %s %s %s %s\n0 %s\n" % (E(0, 1, "0"), E(1, 2, "0.0"), E(2, 3, "-0"), E(3, 4, "0.000"), E(4, 5, "1"),
                                               E(0, 9, "-0.0000000000"))
    t["signs"] = "1 %s %s %s %s %s\n" % (E(0, 1, "-1.5"), E(1, 2, "1."), E(2, 3, ".5"), E(3, 4, "-.5"), E(4, 5, "-7."))
    t["nine_digits"] = "1 %s %s\n" % (E(123456789, 999999999, "1"), E(0, 100000000, "0.5"))
    t["seven_sig"] = "1 %s %s %s %s\n" % (E(0, 1, "0.0001234567"), E(1, 2, "0000001234567"), E(2, 3, "0.001234567"),
                                          E(3, 4, "9999999"))
    t["one_line"] = "1 %s" % E(0, 1, "1")
    return {k: v.encode() for k, v in t.items()}


def slow_lines(has_field):
    """name -> one line outside the device grammar."""
    E = lambda f, i, v: _entry(has_field, f, i, v)  # noqa: E731
    s = {
        "exponent": "1 " + E(0, 1, "1e-3"),
        "eight_sig": "1 " + E(0, 1, "1.2345678"),
        "eleven_frac": "1 " + E(0, 1, "0.00000000001"),
        "nan": "1 " + E(0, 1, "nan"),
        "inf": "1 " + E(0, 1, "inf"),
        "tab": "1 " + E(0, 1, "1") + "\t" + E(1, 2, "1"),
        "plus_value": "1 " + E(0, 1, "+1"),
        "no_value": "1 3:4:" if has_field else "1 4:",
        "ten_digit_id": "1 " + E(0, 1234567890, "1"),
        "minus": "1 " + E(0, 1, "-"),
        "label_float": "1.0 " + E(0, 1, "1"),
        "long_line": ("1 " + E(1, 2, "1")).ljust(65537),
    }
    if has_field:
        s["missing_part"] = "1 3:4"
    return s


# the slow lines the host parser refuses too (`wrong input: ...`)
MALFORMED = ("no_value", "minus", "missing_part")


FAST_BEFORE = "1 %s\n0 %s\n"
FAST_AFTER = "0 %s\n"


def around(has_field, line):
    """(text, offset of `line`) with fast lines before and after it."""
    E = lambda f, i, v: _entry(has_field, f, i, v)  # noqa: E731
    before = FAST_BEFORE % (E(0, 1, "1"), E(1, 2, "0.5"))
    return (before + line + "\n" + FAST_AFTER % E(2, 3, "1")).encode(), len(before)
