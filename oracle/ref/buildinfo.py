"""Writes oracle/_ref/ref_driver.json beside the driver: which reference files and which compiler it was built from.
The file travels with the binary, so tests/golden/gen_reference_pin.py can record it where the reference tree itself
is absent.  TEST INFRASTRUCTURE ONLY.

    python3 ref/buildinfo.py <reference dir> <hipcc> <flags...>    (from oracle/Makefile's `ref` target)
"""
import hashlib
import json
import os
import subprocess
import sys


def main(ref_dir, hipcc, flags):
    files = {}
    src = os.path.join(ref_dir, "src")
    for sub in ("ops", "modules", "utils"):
        d = os.path.join(src, sub)
        for name in sorted(os.listdir(d)):
            if name.endswith(".cuh"):
                with open(os.path.join(d, name), "rb") as f:
                    files[f"src/{sub}/{name}"] = hashlib.sha256(f.read()).hexdigest()
    version = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    here = os.path.dirname(os.path.abspath(__file__))
    own = {}
    for rel in ("ref_driver.hip", "compat/cuda_runtime.h", "compat/curand.h", "compat/curand_kernel.h"):
        with open(os.path.join(here, rel), "rb") as f:
            own["oracle/ref/" + rel] = hashlib.sha256(f.read()).hexdigest()
    json.dump(dict(reference_sha256=files, driver_sha256=own, hipcc_version=version, flags=flags), sys.stdout, indent=1,
              sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3:])
