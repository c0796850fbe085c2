"""The fp32 gather family at the kernel, over the chooser's table (tests/gather_forms.py): every case runs through
acm_conv_bwd_spmm (two or three gathered channels, or one per pass) or acm_spmm_ex (one) with the tables where the case puts them
-- offset bases, odd and padded pitches, [G_L | G_H] adjacent or apart, packed rows, NaN / inf in every pad column and every table
row nobody references, outputs as views of a NaN-filled buffer -- and is compared twice: bit for bit with the integer result on
integer inputs (a dropped, doubled or misplaced neighbour cannot pass), and with float64 under the a-priori bound of fp32
summation in any order on N(0, 1) inputs.  Before a launch the case asks acm_gather_form with the real addresses and requires the
form the table lists; every call runs twice and must repeat itself bit for bit.  The worst error / bound per form is written as
gather_forms.json where ACM_EVIDENCE_DIR says."""
import pytest

import bf16_ref as R
import gather_forms as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_FORMS = set()


@pytest.fixture(autouse=True)
def _evidence():
    yield
    G.dump_evidence(_FORMS)


@pytest.mark.parametrize("name,family", G.PAIRS, ids=[f"{nm}-{fam}" for nm, fam in G.PAIRS])
def test_gather_family_exact_and_bounded(name, family, tune):
    todo = G.cases_for(name, family)
    assert todo
    for case in todo:
        tune(**case.tune)
        reached, worst = G.run_case(name, case, DEV)
        for form in reached:
            kind, lanes, f_arg, ng = form[:4]
            key = f"gather {kind} lanes{lanes} arg{f_arg} ng{ng}" if lanes else f"gather {kind} arg{f_arg} ng{ng}"
            R.note(key, worst, 1.0)
            _FORMS.add("/".join(str(v) for v in form))
        print(f"{name} {case.id}: {reached[0][0]} worst error / bound {worst:.3f}")
