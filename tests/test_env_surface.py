"""The environment surface of the package is what INTEGRATION.md says it is: every NERO_* variable that nero_amd/*.py reads from os.environ
and that nero_amd/csrc/* reads with getenv has a row in the table of INTEGRATION.md ("Environment variables the package reads"), and the
table has no row for a variable nobody reads.  Source text only: nothing is built or imported."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_names():
    names = set()
    for path in sorted(glob.glob(os.path.join(ROOT, 'nero_amd', '*.py'))):
        src = open(path).read()
        # os.environ.get('NAME' ...), os.environ['NAME'], 'NAME' in os.environ; a prefix completed at run time ('NERO_GEMM_' + k.upper())
        # counts as NAME_<...> whatever the table calls the placeholder
        for m in re.finditer(r"os\.environ(?:\.get\(|\[|\.pop\(|\.setdefault\()\s*(['\"])(NERO_[A-Z0-9_]*)\1\s*(\+)?", src):
            names.add(m.group(2) + '<>' if m.group(3) else m.group(2))
        names.update(m.group(2) for m in re.finditer(r"(['\"])(NERO_[A-Z0-9_]+)\1\s+(?:not\s+)?in\s+os\.environ", src))
        assert len(re.findall(r'os\.environ|os\.getenv', src)) == len(re.findall(
            r"os\.environ(?:\.get\(|\[|\.pop\(|\.setdefault\()\s*['\"]NERO_|['\"]NERO_[A-Z0-9_]+['\"]\s+(?:not\s+)?in\s+os\.environ", src)), \
            f'{path}: an environment read this test cannot name'
    for path in sorted(glob.glob(os.path.join(ROOT, 'nero_amd', 'csrc', '*'))):
        src = open(path, errors='replace').read()
        reads = re.findall(r'\bgetenv\s*\(\s*([^)]*)\)', src)
        for arg in reads:
            m = re.fullmatch(r'"(NERO_[A-Z0-9_]+)"\s*', arg)
            assert m, f'{path}: getenv({arg}) is not a literal NERO_* name'
            names.add(m.group(1))
    return names


def _table_names():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    sec = text[text.index('## Environment variables the package reads'):]
    sec = sec[:sec.index('\n## ', 1)]
    rows = re.findall(r'^\| `(NERO_[A-Z0-9_]+)(<[A-Z]+>)?` \|', sec, re.M)
    assert len(rows) == len(set(rows)), rows
    return {name + ('<>' if placeholder else '') for name, placeholder in rows}


def test_environment_table_matches_the_sources():
    read, table = _read_names(), _table_names()
    assert read == table, {'read but not in INTEGRATION.md': sorted(read - table), 'in INTEGRATION.md but not read': sorted(table - read)}
    assert len(read) >= 10                                   # (the scan did find the sources)
