"""The scalar checks of the host layer, written once: "an integer, not a bool, in lo .. hi", "a real number, finite, positive",
"a <ValueClass> (or None)".  Each takes the exception class to raise -- the values of sensor.py raise ValueError, the front ends
EloError for a value and TypeError for a type -- and hands back the checked value; a message is built only where one is raised.
Nothing here imports torch or the library: sensor.py stays importable without either."""
import math


def integer(name, value, kind, lo=None, hi=None):
    """`value` as a python int: anything with __index__ (numpy's integers too) but a bool, within lo .. hi, both inclusive."""
    if isinstance(value, bool) or not hasattr(value, "__index__"):
        raise kind("%s is an integer (got %r)" % (name, value))
    value = value.__index__()
    if (lo is not None and value < lo) or (hi is not None and value > hi):
        raise kind("%s is an integer in %s .. %s (got %d)" % (name, "" if lo is None else lo, "" if hi is None else hi, value))
    return value


def real(name, value, kind, finite=True, positive=False, non_negative=False, takes="any"):
    """`value` as a python float, finite unless finite=False, > 0 with positive, >= 0 with non_negative (a NaN passes none of the
    three).  takes: "any" -- what float() takes, a bool too, and what it does not take is float()'s own TypeError / ValueError, as
    the values of sensor.py have always let it through; "no_bool" -- the same but a bool; "numbers" -- a python int or float
    (numpy.float64 is one) and no bool, anything else is a `kind`."""
    if takes != "any" and (isinstance(value, bool) or (takes == "numbers" and not isinstance(value, (int, float)))):
        raise kind("%s is a number (got %r)" % (name, value))
    out = float(value)
    if out != out or (finite and math.isinf(out)) or (positive and not out > 0) or (non_negative and not out >= 0):
        asked = [word for word, on in (("finite", finite), ("positive", positive), (">= 0", non_negative)) if on]
        raise kind("%s must be %s (got %r)" % (name, " and ".join(asked) or "a number", out))
    return out


def is_a(name, value, cls, kind=TypeError, or_none=False):
    """`value`, an instance of `cls` -- or None, with or_none."""
    if not isinstance(value, cls) and not (or_none and value is None):
        raise kind("%s is a %s%s (got %r)" % (name, cls.__name__, " or None" if or_none else "", type(value).__name__))
    return value
