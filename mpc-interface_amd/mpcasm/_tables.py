"""The plan tables' layout, read from its one statement, ``csrc/plan_tables.h``, once at import.

``VALUES``: name -> int for every enumerator and every ``constexpr int`` / ``int32_t`` of the header;
``ENUMS``: the ordered names of every enum, under the enum's name or, for an anonymous one, its first item's.

This is no C parser.  With the comments stripped it takes, in file order, every ``enum [Name [: type]] {...}`` (an
item without ``= e`` counts on from the one before) and every ``constexpr int|int32_t a = e, b = e;``, an initialiser
being an integer expression over literals, names read so far, parentheses and ``+ - * / % << >> | & ^ ~`` (``/`` as
integer division).  Anything else -- a call, a suffixed literal, another type, an unknown or repeated name, an
``enum`` or ``constexpr`` of another shape -- raises: nothing is skipped.
"""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "csrc", "plan_tables.h")
_DECL = re.compile(r"\benum\s*(\w*)\s*(?::\s*\w+\s*)?\{([^{}]*)\}|\bconstexpr\s+(int|int32_t)\s+([^;{}]*);")


def read(path=HEADER):
    """``(values, enums)`` of the header at ``path``."""
    with open(path) as f:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", " ", f.read(), flags=re.S)
    values, enums = {}, {}

    def declare(name, expr):
        try:
            if not isinstance(expr, int):
                expr = re.sub(r"(?<!\w)[A-Za-z_]\w*", lambda m: str(values[m.group()]), expr)
                if re.fullmatch(r"[\s0-9a-fA-FxX()+\-*/%<>|&^~]+", expr):
                    expr = eval(expr.replace("/", "//"), {"__builtins__": {}})
            if type(expr) is not int or not re.fullmatch(r"[A-Za-z_]\w*", name) or name in values:
                raise ValueError
        except Exception:
            raise ValueError("%s: cannot take %r = %r" % (path, name, expr)) from None
        values[name] = expr
        return expr

    decls = list(_DECL.finditer(text))
    if len(decls) != len(re.findall(r"\b(?:enum|constexpr)\b", text)):
        raise ValueError("%s: an enum or a constexpr of a form the reader does not know" % path)
    for tag, body, _, declarators in (m.groups() for m in decls):
        items = [i.partition("=") for i in (declarators if body is None else body).split(",")]
        if body is not None and not "".join(items[-1]).strip():
            items.pop()                                                # (an enum's trailing comma)
        names, nxt = [], 0
        for name, eq, expr in items:
            nxt = declare(name.strip(), expr if eq or body is None else nxt) + 1
            names.append(name.strip())
        if body is not None and (tag or names[0]) in enums:
            raise ValueError("%s: enum %r twice" % (path, tag))
        if body is not None:
            enums[tag or names[0]] = names
    return values, enums


VALUES, ENUMS = read()
