"""``python -m pyrodigal_amd``: the Prodigal-compatible command line (see :mod:`pyrodigal_amd.cli`)."""
import sys

from .cli import main

if __name__ == "__main__":
    sys.exit(main())
