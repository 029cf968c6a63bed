"""Two textual rewrites that make CUDA C++ sources parse as host C++.

Both are patterns over C syntax and know nothing about any particular file:

  asm("..." "..." : "=r"(out) : "r"(a), "r"(b));
      ->  vro_ref::ptx("......", out, a, b);
      (GCC extended asm with one output: the template strings are joined and
      handed, with the operand expressions, to an interpreter in the stand-in)

  kernel<<<grid, block>>>(args);
      ->  VRO_REF_LAUNCH(kernel, grid, block, args);

`rewrite_tree` copies the sources it is given into a build directory, applies
the rewrites to the copies and insists on the expected number of each; the
copies live under oracle/_ref/ and are never committed.
"""
from __future__ import annotations

import os
import re
import sys

_STRING = re.compile(r'"(?:[^"\\]|\\.)*"')
_OPERAND = re.compile(r'"[^"]*"\s*\(')
_LAUNCH = re.compile(r'\b([A-Za-z_]\w*)\s*<<<\s*([^,<>]+?)\s*,\s*([^<>]+?)\s*>>>\s*\(')


def _matching_paren(text: str, start: int) -> int:
    """Index of the ')' closing the '(' at `start`, skipping string literals."""
    depth, i = 0, start
    while i < len(text):
        c = text[i]
        if c == '"':
            i = _STRING.match(text, i).end()
            continue
        if c == '(':
            depth += 1
        elif c == ')':
            depth -= 1
            if depth == 0:
                return i
        i += 1
    raise ValueError("unbalanced parentheses")


def _split_colons(body: str) -> list:
    """Split an asm statement's body at its top-level ':' separators."""
    parts, depth, i, last = [], 0, 0, 0
    while i < len(body):
        c = body[i]
        if c == '"':
            i = _STRING.match(body, i).end()
            continue
        if c == '(':
            depth += 1
        elif c == ')':
            depth -= 1
        elif c == ':' and depth == 0:
            parts.append(body[last:i])
            last = i + 1
        i += 1
    parts.append(body[last:])
    return parts


def _operands(section: str) -> list:
    """The expressions of  "constraint"(expr), "constraint"(expr) ..."""
    out, i = [], 0
    while True:
        m = _OPERAND.search(section, i)
        if not m:
            return out
        close = _matching_paren(section, m.end() - 1)
        out.append(section[m.end():close].strip())
        i = close + 1


def rewrite_asm(text: str):
    """Replace every GCC extended asm statement; returns (text, count)."""
    out, pos, count = [], 0, 0
    for m in re.finditer(r'\basm\s*(?:volatile\s*)?\(', text):
        if m.start() < pos:
            continue
        close = _matching_paren(text, m.end() - 1)
        parts = _split_colons(text[m.end():close])
        if len(parts) < 3:
            raise ValueError("asm statement without output and input sections")
        template = "".join(s[1:-1] for s in _STRING.findall(parts[0]))
        outs, ins = _operands(parts[1]), _operands(parts[2])
        if len(outs) != 1:
            raise ValueError("asm statement with %d outputs" % len(outs))
        out.append(text[pos:m.start()])
        out.append('vro_ref::ptx("%s", %s)' % (template, ", ".join(outs + ins)))
        out.append("\n" * text.count("\n", m.start(), close))       # keep the line numbers of what follows
        pos = close + 1
        count += 1
    out.append(text[pos:])
    return "".join(out), count


def rewrite_launch(text: str):
    """Replace every triple-chevron kernel launch; returns (text, count)."""
    out, pos, count = [], 0, 0
    for m in _LAUNCH.finditer(text):
        close = _matching_paren(text, m.end() - 1)
        args = text[m.end():close].strip()
        out.append(text[pos:m.start()])
        out.append("VRO_REF_LAUNCH(%s, %s, %s%s)" % (m.group(1), m.group(2), m.group(3), ", " + args if args else ""))
        out.append("\n" * text.count("\n", m.start(), close))
        pos = close + 1
        count += 1
    out.append(text[pos:])
    return "".join(out), count


def rewrite_tree(files: list, dst: str, want_asm: int, want_launch: int) -> None:
    """Copy `files` (paths) into `dst`, rewritten; the totals must match."""
    os.makedirs(dst, exist_ok=True)
    n_asm = n_launch = 0
    for path in files:
        with open(path, encoding="utf-8", errors="surrogateescape") as f:
            text = f.read()
        text, a = rewrite_asm(text)
        text, l = rewrite_launch(text)
        n_asm, n_launch = n_asm + a, n_launch + l
        with open(os.path.join(dst, os.path.basename(path)), "w", encoding="utf-8", errors="surrogateescape") as f:
            f.write(text)
    if (n_asm, n_launch) != (want_asm, want_launch):
        raise RuntimeError("rewrote %d asm statements and %d launches, expected %d and %d"
                           % (n_asm, n_launch, want_asm, want_launch))


if __name__ == "__main__":
    # rewrite.py <dst> <n_asm> <n_launch> <file>...
    rewrite_tree(sys.argv[4:], sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
