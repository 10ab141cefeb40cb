"""What the tests of the libraries' surfaces share: a header's prototypes, a library's exports, the ctypes type of a C argument, a
header compiled alone, and what `make` does in csrc -- its commands, not the Makefile's text."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
CORE = "../libagpl.so"  # as csrc's make names it


def prototypes(path):
    """name -> (return type, [argument, ...]) of every AGPL_API prototype of a header."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {m.group(2): (m.group(1).strip(), [a.strip() for a in m.group(3).split(",") if a.strip()])
            for m in re.finditer(r"AGPL_API\s+([\w\s\*]+?)\b(agpl_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def arguments(path):
    return {name: args for name, (_, args) in prototypes(path).items()}


def arities(path):
    return {name: len(args) for name, args in arguments(path).items()}


def ctype(arg):
    if "*" in arg:
        return C.c_void_p
    return {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}[arg.split()[0]]


def exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return sorted(set(re.findall(r" T (agpl_\w+)", out)))


def header_compiles_alone(header, main_body, tmp_path):
    """A C11 and a C++17 unit that include only `header` and whose main is `main_body` compile without a warning."""
    done = 0
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        if shutil.which(cc) is None:
            continue
        f = tmp_path / f"t.{ext}"
        f.write_text('#include "%s"\nint main(void) { %s }\n' % (header, main_body))
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, "-c", str(f), "-o",
                               str(tmp_path / f"t_{ext}.o")])
        done += 1
    assert done, "no host compiler"


@functools.lru_cache(maxsize=None)
def _make(*args):
    return subprocess.check_output(["make", "-n"] + list(args), cwd=CSRC).decode().splitlines()


@functools.lru_cache(maxsize=None)
def build_commands(*targets):
    """(compile command per object, link command per library) of `make -n -B [targets]` in csrc, each in the order make runs them."""
    compiles, links = {}, {}
    for line in _make("-B", *targets):
        words = line.split()
        if "-c" in words:
            assert words[-1] not in compiles, line
            compiles[words[-1]] = line  # ... -c agpl_X.hip -o agpl_X.o
        elif "-shared" in words:
            lib = words[words.index("-o") + 1]
            assert lib not in links, line
            links[lib] = line
    return compiles, links


def objects(command):
    return [w for w in command.split() if w.endswith(".o")]


def link_tail(lib):
    """An extension's link command without its output and its object(s): what is the same for every extension."""
    return [w for w in build_commands()[1][lib].split() if w != lib and not w.endswith(".o")]


def linked_like(lib, *others):
    """`lib` is linked after libagpl.so, against it, and by the same command as `others` but for the names."""
    order = list(build_commands(lib)[1])
    assert order.index(CORE) < order.index(lib), order
    tail = link_tail(lib)
    assert "-L.." in tail and "-lagpl" in tail and "-Wl,-rpath,'$ORIGIN'" in tail, tail
    for other in others:
        assert link_tail(other) == tail, other
    return True


def links_exactly(lib, *objs):
    """The default target links `lib` from exactly `objs`, each compiled from the source of its name and in no other library;
    `make clean` removes them and it."""
    compiles, links = build_commands()
    assert objects(links[lib]) == list(objs), links[lib]
    for obj in objs:
        assert " -c %s.hip -o %s" % (obj[:-2], obj) in compiles[obj], compiles[obj]
    for other, command in links.items():
        assert other == lib or not set(objs) & set(objects(command)), other
    cleaned = set(w for line in _make("clean") for w in line.split())
    assert set(objs) | {lib} <= cleaned, cleaned
    return True


def contraction_off(obj):
    return "-ffp-contract=off" in build_commands()[0][obj].split()


def recompiled_by(header):
    """The objects that a change to `header` (a path relative to csrc) compiles again on a built tree."""
    return {line.split()[-1] for line in _make("-W", header) if " -c " in line}
