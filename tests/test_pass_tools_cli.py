"""The per-pass timing tools (tools/<pass>_bench.py) keep their command lines: --help of each names exactly the options recorded in
golden/pass_tools_cli.json (written from the tools as they were before tools/pass_frames.py), importing one and printing its help never
touches the GPU, and no tool imports another tool."""
import ast
import glob
import importlib
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)

with open(os.path.join(ROOT, "tests", "golden", "pass_tools_cli.json")) as _f:
    OPTIONS = json.load(_f)


@pytest.mark.parametrize("tool", sorted(OPTIONS))
def test_help_names_the_recorded_options(tool, capsys, monkeypatch):
    import torch

    monkeypatch.setenv("COLUMNS", "500")  # one line per option, so no option name is broken at a hyphen
    module = importlib.import_module(tool + "_bench")
    with pytest.raises(SystemExit) as e:
        module.main(["--help"])
    assert e.value.code == 0
    assert sorted(set(re.findall(r"(?<![\w-])--[a-z][a-z-]*", capsys.readouterr().out))) == OPTIONS[tool]
    assert not torch.cuda.is_initialized()


def test_every_tool_is_recorded():
    assert sorted(os.path.basename(p)[: -len("_bench.py")] for p in glob.glob(os.path.join(TOOLS, "*_bench.py"))) == sorted(OPTIONS)


def test_no_tool_imports_another_tool():
    for path in glob.glob(os.path.join(TOOLS, "*_bench.py")):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, (ast.Import, ast.ImportFrom)) else []
            if isinstance(node, ast.ImportFrom) and node.module:
                names.append(node.module)
            for name in names:
                assert not name.split(".")[-1].endswith("_bench"), f"{os.path.basename(path)} imports {name}"
