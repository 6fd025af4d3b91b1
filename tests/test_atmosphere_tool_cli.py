"""tools/atmosphere_timing.py keeps its command line and its row schema: --help names exactly the options below, importing it and printing its
help never touches the GPU, it imports no other tool, and the fields of its rows are those recorded in golden/atmosphere_tool_cli.json.  (It
is not named *_bench.py: golden/pass_tools_cli.json records the ten tools as they were before tools/pass_frames.py, and test_pass_tools_cli.py
holds the tools directory to that record.)"""
import ast
import importlib
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)

with open(os.path.join(ROOT, "tests", "golden", "atmosphere_tool_cli.json")) as f:
    GOLDEN = json.load(f)


def test_help_names_the_options(capsys, monkeypatch):
    import torch

    monkeypatch.setenv("COLUMNS", "500")  # one line per option, so no option name is broken at a hyphen
    module = importlib.import_module("atmosphere_timing")
    with pytest.raises(SystemExit) as e:
        module.main(["--help"])
    assert e.value.code == 0
    assert sorted(set(re.findall(r"(?<![\w-])--[a-z][a-z-]*", capsys.readouterr().out))) == GOLDEN["options"]
    assert not torch.cuda.is_initialized()


def _tree():
    path = os.path.join(TOOLS, "atmosphere_timing.py")
    with open(path) as f:
        return ast.parse(f.read(), path)


def test_it_imports_no_other_tool():
    imported = set()
    for node in ast.walk(_tree()):
        if isinstance(node, ast.Import):
            imported |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.module:
            imported.add(node.module.split(".")[0])
    tools = {os.path.splitext(name)[0] for name in os.listdir(TOOLS) if name.endswith(".py")} - {"pass_frames", "atmosphere_timing"}
    assert not imported & tools, imported & tools


def test_row_schema():
    """The keys of the one dict the tool reports, read from its source, and the rows it names."""
    rows = [node for node in ast.walk(_tree()) if isinstance(node, ast.Dict) and any(isinstance(k, ast.Constant) and k.value == "workload" for k in node.keys)]
    assert len(rows) == 1
    assert [k.value for k in rows[0].keys] == GOLDEN["row_fields"]
    text = ast.unparse(_tree())
    for name in GOLDEN["calls"] + GOLDEN["extents"]:
        assert repr(name) in text, name
