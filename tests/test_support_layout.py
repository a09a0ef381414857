"""No test module imports a test module: what two of them share lives in a plain support module (gpu_support, orc, scene_matrix,
the *_ref modules), so running one file loads that file and the support it names, and a test file's functions are its own."""
import glob
import os
import re

TESTS = os.path.dirname(os.path.abspath(__file__))
# `import test_x`, `from test_x import y`, `import a, test_x`, and the same by name through __import__ / import_module
IMPORTS_A_TEST = re.compile(r"""^\s*(from\s+test_\w*\s+import\b|import\s+([\w.]+\s*(as\s+\w+\s*)?,\s*)*test_\w)|(__import__|import_module)\(\s*["']test_""")


def test_no_test_module_imports_a_test_module():
    found = []
    for path in sorted(glob.glob(os.path.join(TESTS, "**", "*.py"), recursive=True)):
        with open(path) as f:
            for n, line in enumerate(f, 1):
                if IMPORTS_A_TEST.search(line):
                    found.append(f"{os.path.relpath(path, TESTS)}:{n}: {line.strip()}")
    assert not found, "a test module is imported by:\n" + "\n".join(found)
