"""The weight inventory equals the reference modules' state_dict(): key order and shapes as the reference's MegaG /
MegaPLM / MegaADM built from its configs/*.yaml report them (tests/golden/ref_state_dict_shapes.json, written by
oracle/make_golden.py --extra-host)."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inventories_equal_reference_state_dicts():
    from megatts2_amd import config as C
    from megatts2_amd import weights
    with open(os.path.join(ROOT, "tests", "golden", "ref_state_dict_shapes.json")) as f:
        ref = json.load(f)
    for name, inv in (("G", weights.inventory_g(C.production_g())), ("plm", weights.inventory_plm(C.production_plm())),
                      ("adm", weights.inventory_adm(C.production_adm()))):
        sd = ref[name]
        assert [k for k, _ in sd] == list(inv.keys())
        for k, shape in sd:
            assert tuple(shape) == tuple(inv[k]), k
