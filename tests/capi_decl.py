"""What include/convdr_hip.h declares, for the CPU tests that hold the ctypes table (convdr_amd/_lib.py: _SIGNATURES) against it."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "convdr_hip.h")


def params(name):
    """The parameter list of the declared entry `name`, comments stripped: the text between its parentheses.  LookupError for a
    name the header does not declare; ValueError for a declaration this simple pattern cannot read (nested parentheses: a
    function-pointer parameter)."""
    with open(HEADER) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    found = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
    if found is None:
        raise LookupError("%s is not declared in include/convdr_hip.h" % name)
    if "(" in found.group(1):
        raise ValueError("%s: nested parentheses in the parameter list" % name)
    return found.group(1)
