"""Every MAGICKHIP_* option the library reads has a user in the tree: no GPU needed.

An option name in imagemagick_amd/csrc stays only if it is one of the deployment knobs that runtime.cpp's
user_option() lists, or if a file under tests/ or tools/, or bench.py, names it.  A name nothing sets selects code
that nothing runs: remove the read, and whatever only that read could reach."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "imagemagick_amd", "csrc")
NAME = re.compile(r'"(MAGICKHIP_[A-Z0-9_]+)"')


def read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def source_option_names():
    names = {}
    for entry in sorted(os.listdir(CSRC)):
        if entry.endswith((".hip", ".cpp", ".hpp")):
            for name in NAME.findall(read(os.path.join(CSRC, entry))):
                names.setdefault(name, entry)
    return names


def deployment_names():
    body = re.search(r"static const char \*const deployment\[\]=\{(.*?)\};", read(os.path.join(CSRC, "runtime.cpp")),
                     re.S)
    assert body, "user_option()'s deployment array was not found in runtime.cpp"
    return set(NAME.findall(body.group(1)))


def user_text():
    parts = [read(os.path.join(ROOT, "bench.py"))]
    for top in ("tests", "tools"):
        for folder, _, files in os.walk(os.path.join(ROOT, top)):
            if "__pycache__" in folder:
                continue
            for entry in files:
                path = os.path.join(folder, entry)
                if os.path.abspath(path) != os.path.abspath(__file__) and not entry.endswith((".pyc", ".so", ".o")):
                    parts.append(read(path))
    return "\n".join(parts)


def test_every_option_read_is_a_deployment_knob_or_has_a_user_in_the_tree():
    names = source_option_names()
    deployment = deployment_names()
    assert len(names) > 20 and len(deployment) >= 8, "the sources were not parsed"
    used = set(re.findall(r"MAGICKHIP_[A-Z0-9_]+", user_text()))
    orphans = sorted(n for n in names if n not in deployment and n not in used)
    assert not orphans, (
        "option names read in imagemagick_amd/csrc that nothing sets: %s.  An option stays only if user_option() in "
        "runtime.cpp lists it as a deployment knob or a file under tests/, tools/ or bench.py names it; otherwise "
        "remove the read and the code only it could reach."
        % ", ".join("%s (%s)" % (n, names[n]) for n in orphans))
