"""The part of tests/test_gpu_maintenance_drawn.py that runs in a process of its own: at the default grid every wavefront of k_decay holds ONE block
until a map exceeds 32768 blocks, so the bookkeeping that keeps 64 blocks per wavefront in lanes never runs on a small map.  NVBX_DECAY_GRID is
read when a mapper is created (the process of its own keeps a fault away from the rest of the file); with NVBX_DECAY_GRID=1 in the environment the decay launch is one workgroup, whose eight wavefronts take 64 blocks each per
round.  Run as  python tests/maintenance_child.py : case A (the weight ladder, all four variants) and the five-round conservation sequence against
the model, then the marker on stdout."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OK_MARKER = "MAINTENANCE_CHILD_OK"


def main():
    assert os.environ.get("NVBX_DECAY_GRID") == "1", "the child is meant to run with NVBX_DECAY_GRID=1"
    from isaac_ros_nvblox_amd import mapper as M
    import maintenance_cases as MC
    for variant in MC.DECAY_VARIANTS:
        case = MC.case_a("dyadic", variant)
        side = MC.ProductSide(M, MC.params(M, case))
        MC.run_case(case, side, after_hook=MC.lookup_hook(side))
        side.close()
        print("case %s: ok" % case.name, flush=True)
    side = MC.conservation_rounds(M)[0]
    side.close()
    print("conservation rounds: ok", flush=True)
    print(OK_MARKER, flush=True)


if __name__ == "__main__":
    main()
