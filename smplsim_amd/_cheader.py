"""Reader of the public C headers under include/: structs, prototypes and integer constants as plain Python data.

parse(text, name) understands the plain C these headers are written in and nothing more.  It never skips: whatever it does
not recognise raises HeaderError with the header's name and the offending text.

  preprocessor   #include <...>; the include guard; `#ifdef __cplusplus` around `extern "C" {` and `}`; `#define NAME <integer>`,
                 bare or as the default inside `#ifndef NAME ... #endif`.  Between declarations only.
  declarations   enum { A, B = 3, C = NAME } and typedef enum { ... } name;  typedef struct [tag] { fields } name;
                 struct tag;  typedef struct tag name;  ret name(type param, ...);  ret name(void);
  declarators    a named object with its own stars and one array bound: `const double *kp, *kd`, `double solref[2], margin`,
                 `const char *const *names`, `ss_model **out`.  No bit-fields, function pointers or unnamed parameters.
  types          the scalars of SCALARS, void, and the structs and handles declared earlier in the same header.

A C type comes back as a string in one spelling: the specifiers as written, then the stars (`const char *const *`,
`ss_model **`), then the array bound (`double[5]`).
"""
import collections
import re

SCALARS = ("int", "int32_t", "int64_t", "float", "double", "size_t", "uint8_t", "char", "unsigned long long")
_TYPE_WORDS = {w for s in SCALARS for w in s.split()} | {"const", "struct", "void"}

# structs: name -> [(field, type)];  functions: name -> (return type, [parameter types]);  constants: name -> int, enumerators
# and defines alike;  opaque: the handles, declared but never defined.  Each in the order of the header.
Header = collections.namedtuple("Header", "structs functions constants opaque")


class HeaderError(ValueError):
    pass


def parse(text, name="<header>"):
    def fail(what, where):
        raise HeaderError(f"{name}: {what}: {' '.join(where.split())!r}")

    h = Header({}, {}, {}, [])
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda c: " " + "\n" * c.group().count("\n"), text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*", "#", text, flags=re.M)
    guard = re.fullmatch(r"\s*#ifndef (\w+)\s*?\n#define \1[ \t]*\n(.*)\n#endif\s*", text, re.S)
    text = guard.group(2) if guard else text
    text = re.sub(r"^#include[ \t]*<[\w./]+>[ \t]*$", "", text, flags=re.M)
    text = re.sub(r'^#ifdef __cplusplus\s*?\n\s*(extern "C" \{|\})\s*?\n#endif[ \t]*$', "", text, flags=re.M)
    text = re.sub(r"^#ifndef (\w+)\s*?\n(#define \1 [^\n]*)\n#endif[ \t]*$", r"\2", text, flags=re.M)
    text = re.sub(r"^#define (\w+)[ \t]+(\S+)[ \t]*$", r"enum { \1 = \2 };", text, flags=re.M)     # an integer define reads like an enumerator
    if "#" in text:
        fail("preprocessor line not understood (or inside a declaration)", re.search(r"#[^\n]*", text).group())

    def constant(cname, value, where):
        try:
            h.constants[cname] = h.constants[value] if value in h.constants else int(value, 0)
        except ValueError:
            fail("value that is neither an integer nor a constant declared earlier", where)
        return h.constants[cname]

    def declarators(decl, where, void_ok=False):
        """`specifiers declarator, declarator, ...` -> [(name, type)]"""
        words, known = re.findall(r"\w+|[^\w\s]", decl), set(h.structs) | set(h.opaque)
        n = next((i for i, w in enumerate(words) if w not in _TYPE_WORDS and w not in known), len(words))
        base = " ".join(w for w in words[:n] if w not in ("const", "struct"))
        if base not in known and ("struct" in words[:n] or base not in SCALARS + ("void",)):
            fail("unknown type", decl if decl.strip() else where)
        out = []
        for d in "".join(w if w in "*[]," else f" {w} " for w in words[n:]).split(","):
            m = re.fullmatch(r"((?:\*|const|\s)*?)\s*(?!const\b)(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", d)
            if not m or (base == "void" and "*" not in m.group(1) and not void_ok):
                fail("declarator not understood", decl)
            stars = "".join("*" if t == "*" else "const " for t in re.findall(r"\*|const", m.group(1))).strip()
            out.append((m.group(2), " ".join(words[:n]) + (" " + stars if stars else "") + (f"[{m.group(3)}]" if m.group(3) else "")))
        return out

    depth, start, stmts = 0, 0, []
    for i, ch in enumerate(text):                                     # statements: the text between the semicolons outside braces
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            stmts.append(text[start:i].strip())
            start = i + 1
    if text[start:].strip():
        fail("declaration without its closing ';'", text[start:])
    for stmt in stmts:
        if (m := re.fullmatch(r"(?:typedef\s+)?enum\s*(?:\w+\s*)?\{(.*)\}\s*\w*", stmt, re.S)):
            nxt = 0
            for item in m.group(1).split(","):
                if not (e := re.fullmatch(r"\s*(\w+)\s*(?:=\s*(\S+)\s*)?", item)):
                    fail("enumerator not understood", stmt)
                nxt = constant(e.group(1), e.group(2) or str(nxt), stmt) + 1
        elif (m := re.fullmatch(r"typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)", stmt)) and m.group(1) in ("", m.group(3)):
            h.structs[m.group(3)] = [f for decl in m.group(2).split(";") if decl.strip() for f in declarators(decl, stmt)]
        elif (m := re.fullmatch(r"typedef\s+struct\s+(\w+)\s+\1|struct\s+(\w+)", stmt)):
            h.opaque.extend({m.group(1) or m.group(2)} - set(h.opaque))
        elif (m := re.fullmatch(r"(?!typedef\b)([^(){}]*?)(\w+)\s*\(([^(){}]*)\)", stmt)) and m.group(2) not in h.functions:
            params = [] if m.group(3).strip() == "void" else [t for p in m.group(3).split(",") for _, t in declarators(p, stmt)]
            h.functions[m.group(2)] = (declarators(m.group(1) + " result", stmt, True)[0][1], params)
        else:
            fail("declaration not understood", stmt)
    return h
