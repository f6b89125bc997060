"""The inference script, test.py at the repository root, loaded as a module: it is a script, not part of the package, so
the tests that call its functions load it by path."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_cli(name="codlad_cli"):
    """A fresh module object of test.py (its module-level tables start empty for every caller)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def option(cli, flag):
    """How build_parser() declares `flag`: its argparse action (type, nargs, const, default, choices)."""
    return next(a for a in cli.build_parser()._actions if flag in a.option_strings)
