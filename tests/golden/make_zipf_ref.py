"""Pins the golden zipf draws to the REFERENCE's generator (run from repo
root: `python tests/golden/make_zipf_ref.py [--write]`).

Builds oracle/_ref/zipf_ref (`make -C oracle ref`: the reference's own
test/zipf.h compiled by path from the reference checkout with
-ffp-contract=off and a driver of ours, oracle/zipf_ref_main.cpp), draws 256
values for every (n, theta, seed) of tests/golden/generators.json, and checks
them against the fixture (the oracle's restatement, make_golden.py) — with
--write it stores the reference's draws into the fixture instead.  The same
for tests/golden/zipf_reference.json, the reference's recorded output that
tests/test_oracle.py checks the oracle against where no reference checkout
is at hand: the golden cases' 256 draws and FURTHER's 2000 draws each.  Exit
status 0 = the fixtures equal the reference's output."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIX = os.path.join(ROOT, "tests", "golden", "generators.json")
REC = os.path.join(ROOT, "tests", "golden", "zipf_reference.json")
BIN = os.path.join(ROOT, "oracle", "_ref", "zipf_ref")
# further (n, theta, seed) cases, among them C3's and C5's generators (theta
# 0.99 over 2^26 and 2^31 items)
FURTHER = [(64 << 20, 0.99, 0x5EED0007), (1 << 31, 0.99, 12345), (4000, 0.99, 1),
           (1 << 20, 0.3, 99), (10, 0.0, 3)]
FURTHER_DRAWS = 2000


def reference_draws(n, theta, seed, count):
    out = subprocess.run([BIN, str(n), repr(float(theta)), str(seed), str(count)],
                         capture_output=True, text=True, check=True).stdout
    return [int(x) for x in out.split()]


def main():
    rc = subprocess.call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    if rc != 0 and not os.path.isfile(BIN):
        return rc
    # (a binary built earlier serves where the checkout has gone since)
    print("zipf_ref: " + ("built from the reference checkout, or up to date with it" if rc == 0
                          else "`make ref` failed, using the binary built earlier"))
    gen = json.load(open(FIX))
    ok = True
    for z in gen["zipf"]:
        ref = reference_draws(z["n"], z["theta"], z["seed"], len(z["draws"]))
        same = ref == z["draws"]
        print(f"n={z['n']} theta={z['theta']} seed={z['seed']:#x}: "
              f"{'equal' if same else 'DIFFERENT'}")
        ok = ok and same
        z["draws"] = ref
    rec = {"golden": [dict(z) for z in gen["zipf"]],
           "further": [{"n": n, "theta": theta, "seed": seed,
                        "draws": reference_draws(n, theta, seed, FURTHER_DRAWS)}
                       for n, theta, seed in FURTHER]}
    try:
        same = json.load(open(REC)) == rec
    except (OSError, ValueError):
        same = False
    print(f"zipf_reference.json: {'equal' if same else 'DIFFERENT'}")
    ok = ok and same
    if "--write" in sys.argv:
        with open(FIX, "w") as f:
            json.dump(gen, f)
        with open(REC, "w") as f:
            json.dump(rec, f)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
