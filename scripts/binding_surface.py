"""The Python surface of a built tree's gbrl_cpp, for showing that a change of the binding left every name and docstring alone.

    python3 scripts/binding_surface.py [ROOT] [> FILE]      # ROOT: the root of a built tree (default: this one)

Needs no GPU.  Prints one JSON document: for the module, GBRL and PreparedDataset, every attribute name (those with a leading underscore
included) with its __doc__, the names sorted -- the order of a __dict__ follows the order the methods were registered in and is not part of
the surface.  Two builds have the same surface when the two outputs are the same bytes (compare their sha256sum).
"""
import importlib.util
import json
import os
import sys


def load(root):
    spec = importlib.util.spec_from_file_location("gbrl_amd_surface", os.path.join(root, "gbrl_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(root, "gbrl_amd")])
    pkg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pkg)
    return pkg.gbrl_cpp


def docs(obj):
    out = {}
    for name in sorted(vars(obj)):
        doc = getattr(getattr(obj, name), "__doc__", None)
        out[name] = doc if isinstance(doc, str) else None
    return out


def surface(root):
    m = load(root)
    return {"gbrl_cpp": {"__doc__": m.__doc__, "attributes": docs(m)},
            "GBRL": {"__doc__": m.GBRL.__doc__, "attributes": docs(m.GBRL)},
            "PreparedDataset": {"__doc__": m.PreparedDataset.__doc__, "attributes": docs(m.PreparedDataset)}}


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    print(json.dumps(surface(root), indent=1, sort_keys=True))
