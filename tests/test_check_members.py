"""tools/check_members.py in the CPU suite: the host layer (drop-in classes + msorb_host:: templates) may only touch members that
exist and are public in the reference's include/ headers — it is compiled here against stand-ins, so this is the only place a drift
between the stand-ins and the real headers shows before integration.  The reference is not part of the repository: the checks run
on tests/golden/reference_members.json, the declarations the tool parsed from those headers (`tools/check_members.py --write-table`)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_host_layer_matches_reference_headers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_members.py"), "--stored"], capture_output=True, text=True)
    rep = json.loads(r.stdout)
    assert rep["problems"] == [], "\n".join(rep["problems"])
    assert r.returncode == 0
    assert rep["member_accesses_checked"] >= 80
    assert rep["type_comparisons"] >= 120
    for c in ("Frame", "KeyFrame", "MapPoint", "ORBextractor", "ORBmatcher", "GeometricCamera"):
        assert rep["classes_parsed"][c] > 10


def test_parser_sees_access_and_kind():
    """The checker has teeth: it tells protected from public and data from functions (KeyFrame::NLeft is protected and only
    reachable through GetNLeft(); Frame's feature arrays are public, KeyFrame's are not)."""
    import check_members as cm
    classes = cm.load_table()
    assert "public" not in cm.lookup(classes, "KeyFrame", "NLeft")["access"]
    e = cm.lookup(classes, "KeyFrame", "GetNLeft")
    assert e["kind"] == "function" and "public" in e["access"] and e["arity"] == {0}
    assert "public" in cm.lookup(classes, "Frame", "mvKeysUn")["access"] and cm.lookup(classes, "Frame", "mvKeysUn")["kind"] == "data"
    assert "public" not in cm.lookup(classes, "KeyFrame", "mvKeysUn")["access"]
    assert "public" not in cm.lookup(classes, "MapPoint", "mfMaxDistance")["access"]
    assert cm.lookup(classes, "MapPoint", "NoSuchMember") is None
    assert cm.lookup(classes, "ORBmatcher", "SearchByProjection")["arity"] >= {4, 5, 6, 8}
    assert "protected" in cm.lookup(classes, "ORBmatcher", "mfNNratio")["access"]
    assert cm.lookup(classes, "ORBextractor", "mvImagePyramid")["access"] == {"public"}


def test_type_drift_is_caught():
    """The type check has teeth: declarations in which Frame::mvKeysUn became a vector of Point2f, the feature grid lost a nesting
    level and GetIndexInKeyFrame returns a plain int — parsed like the headers and put in place of the stored ones — must fail,
    member by member."""
    import check_members as cm
    classes = cm.load_table()
    drift = {"Frame": "public: std::vector<cv::Point2f> mvKeysUn;",
             "KeyFrame": "public: std::vector<std::vector<size_t> > GetFeatureGrids();",
             "MapPoint": "public: int GetIndexInKeyFrame(std::shared_ptr<KeyFrame> pKF);"}
    for cls, decl in drift.items():
        classes[cls]["members"].update(cm.members("class", decl))
    problems, _ = cm.type_check(classes, cm.host_accesses())
    text = "\n".join(problems)
    assert "Frame::mvKeysUn" in text and "KeyFrame::GetFeatureGrids" in text and "MapPoint::GetIndexInKeyFrame" in text
    assert len(problems) >= 4      # EXPECTED_TYPES and the stand-in comparison both object to mvKeysUn
