"""pytest plugin of tools/control_pin_mutations.py (loaded with -p, in every xdist worker too): points tests/lsn_testlib at the mutated oracle and
transmitter libraries named by LSN_MUTANT_ORACLE / LSN_MUTANT_TXGEN."""
import os
import sys


def pytest_configure(config):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import lsn_testlib
    lsn_testlib.ORACLE_SO = os.environ["LSN_MUTANT_ORACLE"]
    lsn_testlib.TXGEN_SO = os.environ["LSN_MUTANT_TXGEN"]
