"""tools/fxaa_timing.py keeps its command line: --help names exactly the options below, importing it and printing its help never touches the
GPU, and it imports no other tool.  (It is not named *_bench.py: golden/pass_tools_cli.json records the ten tools as they were before
tools/pass_frames.py, and a new tool has no such record.)"""
import ast
import importlib
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)

OPTIONS = ["--hbm-tbs", "--help", "--meshlets", "--out", "--size", "--steps", "--transparent", "--warmup"]


def test_help_names_the_options(capsys, monkeypatch):
    import torch

    monkeypatch.setenv("COLUMNS", "500")  # one line per option, so no option name is broken at a hyphen
    module = importlib.import_module("fxaa_timing")
    with pytest.raises(SystemExit) as e:
        module.main(["--help"])
    assert e.value.code == 0
    assert sorted(set(re.findall(r"(?<![\w-])--[a-z][a-z-]*", capsys.readouterr().out))) == OPTIONS
    assert not torch.cuda.is_initialized()


def test_it_imports_no_other_tool():
    path = os.path.join(TOOLS, "fxaa_timing.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.module:
            imported.add(node.module.split(".")[0])
    tools = {os.path.splitext(name)[0] for name in os.listdir(TOOLS) if name.endswith(".py")} - {"pass_frames", "fxaa_timing"}
    assert not imported & tools, imported & tools
