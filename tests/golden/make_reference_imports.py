"""Records which ``Multimodal_AUV.*`` names the reference package's files import from each
other -> tests/golden/reference_imports.json (names only, no code).

    python tests/golden/make_reference_imports.py /path/to/Multimodal-AUV/src/Multimodal_AUV

``files``: for every file of the reference package with such imports, its import statements as
[module, [names], deferred] (deferred = inside a function body, so not run at import time);
``packages``: the package directories (those with an ``__init__.py``); ``api``: the names the
reference's top ``__init__.py`` re-exports from ``functions.functions``.
tests/test_reference_entry_cpu.py rebuilds a stand-in package tree from this list."""
import ast
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_imports.json")


def _imports(path):
    tree = ast.parse(open(path, encoding="utf-8-sig").read())
    deferred = set()
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
            deferred.update(id(n) for n in ast.walk(node) if n is not node)
    rows = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level == 0 and node.module and \
                node.module.startswith("Multimodal_AUV."):
            rows.append([node.module, sorted(a.name for a in node.names), id(node) in deferred])
        elif isinstance(node, ast.Import):
            for a in node.names:
                if a.name.startswith("Multimodal_AUV."):
                    rows.append([a.name, [], id(node) in deferred])
    return sorted(rows)


def main(ref_pkg):
    files, packages = {}, []
    for d, dirs, fs in os.walk(ref_pkg):
        dirs[:] = sorted(x for x in dirs if x != "__pycache__")
        if "__init__.py" in fs:
            packages.append(os.path.relpath(d, ref_pkg).replace(os.sep, "/"))
        for f in sorted(fs):
            if f.endswith(".py"):
                rows = _imports(os.path.join(d, f))
                if rows:
                    files[os.path.relpath(os.path.join(d, f), ref_pkg).replace(os.sep, "/")] = rows
    init = ast.parse(open(os.path.join(ref_pkg, "__init__.py"), encoding="utf-8-sig").read())
    api = sorted(a.name for n in ast.walk(init) if isinstance(n, ast.ImportFrom)
                 and (n.module or "").endswith("functions") for a in n.names)
    with open(OUT, "w") as f:
        json.dump({"files": files, "packages": sorted(packages), "api": api}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"{len(files)} files, {len(packages)} packages, api {api} -> {OUT}")


if __name__ == "__main__":
    main(sys.argv[1])
