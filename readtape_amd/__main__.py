"""`python -m readtape_amd <options> <basefilename>[.ext]`: the command line (readtape_amd/cli.py)."""
import sys

from .cli import main

if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
