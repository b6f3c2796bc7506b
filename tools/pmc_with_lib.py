"""tools/pmc_summary.py against an alternative build of the library (development A/B tool): the same as setting MDX_LIB for it, so
that the three PMC passes run `tools/bench_with_lib.py <lib>` instead of bench.py.
    python tools/pmc_with_lib.py moldiff_amd/libmoldiff_hip_x.so out.json [bench args]"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.exit(subprocess.run([sys.executable, os.path.join(HERE, 'pmc_summary.py')] + sys.argv[2:],
                        env=dict(os.environ, MDX_LIB=os.path.abspath(sys.argv[1]))).returncode)
