"""pmctf_records, the one reader and writer of the nine sidecar records of a bitstream folder: every record is written
valid by its module's own writer, then its reader must refuse each kind of damage with a ValueError that starts with the
path, and give its documented answer for a file that is not there.  No GPU, no codec."""
import json
import os

import pytest

import pmctf_chroma
import pmctf_gop
import pmctf_layers
import pmctf_rate
import pmctf_records
import pmctf_scale
import pmctf_seq

CODEC = {"num_me_stages": 3, "precision": "fp32", "aten_threads": 1}
HASH = {"y": 1, "cb": 2, "cr": 3, "frame": 4}
MISSING_IS_AN_ERROR = object()


def _sequence(folder, gop=4):
    return pmctf_gop.write_sequence_header(folder, width=64, height=48, frame_num=gop, gop=gop, q_index=3, psize=128,
                                           me_downsample=1, ll_order="plane", **CODEC)


def _structure(folder):
    return pmctf_seq.write_gop_structure(folder, width=64, height=48, frame_num=4, max_gop=4, q_index=3, ll_order="plane",
                                         gops=[{"first": 0, "size": 4, "me_downsample": 1, "psize": 128}], **CODEC)


def _rate(folder):
    record = {"alloc": 400, "budget": 400, "q_index": 10, "fits": True, "bits": 320, "trials": [(10, 320)], "credit": 80}
    return pmctf_rate.write_rate_record(folder, pmctf_rate.Controller(1000, 10), [record])


def _layer_hashes(folder):
    # write_layer_hashes decodes the folder on the GPU; its record for a sequence of one GOP of two pictures, by hand
    _sequence(folder, gop=2)
    record = {"format_version": pmctf_layers.LAYER_HASH_FORMAT_VERSION, "level": "u8", "layers": {"1": [dict(HASH, index=0)]}}
    return pmctf_records.write_record(os.path.join(folder, pmctf_layers.LAYER_HASHES), record, indent=1)


def _layer_extract(folder):
    src = folder + ".src"
    os.makedirs(os.path.join(src, pmctf_gop.gop_folder(0)))
    _sequence(src, gop=2)
    for name in pmctf_layers.layer_file_names(2, 1):
        open(os.path.join(src, pmctf_gop.gop_folder(0), name), "wb").close()
    pmctf_layers.extract_layer(src, folder, 1)
    return os.path.join(folder, pmctf_layers.LAYER_EXTRACT)


# name, writer(folder) -> path, reader(folder), the exact field set is checked, the answer for a missing file
RECORDS = [
    ("sequence.json", _sequence, pmctf_gop.read_sequence_header, False, MISSING_IS_AN_ERROR),
    ("picture_format.json", lambda d: pmctf_gop.write_picture_format(d, 10), pmctf_gop.read_picture_format, True, 8),
    ("picture_hashes.json", lambda d: pmctf_gop.write_picture_hashes(d, "u8", [HASH] * 4),
     lambda d: pmctf_gop.read_picture_hashes(d, 4), True, MISSING_IS_AN_ERROR),
    ("gop_structure.json", _structure, pmctf_seq.read_gop_structure, True, MISSING_IS_AN_ERROR),
    ("rate_control.json", _rate, pmctf_rate.read_rate_record, True, MISSING_IS_AN_ERROR),
    ("layer_hashes.json", _layer_hashes, pmctf_layers.read_layer_hashes, True, MISSING_IS_AN_ERROR),
    ("layer_extract.json", _layer_extract, pmctf_layers.read_layer_extract, True, None),
    ("display_format.json", lambda d: pmctf_scale.write_display_format(d, 64, 48), pmctf_scale.read_display_format, True, None),
    ("source_format.json", lambda d: pmctf_chroma.write_source_format(d, "444", "center", (25, 1)),
     pmctf_chroma.read_source_format, True, None),
]


@pytest.mark.parametrize("name,write,read,exact,missing", RECORDS, ids=[r[0] for r in RECORDS])
def test_every_reader_refuses_damage_and_names_the_path(tmp_path, name, write, read, exact, missing):
    folder = str(tmp_path / "bins")
    os.makedirs(folder, exist_ok=True)
    path = write(folder)
    assert path == os.path.join(folder, name)
    text = open(path).read()
    valid = json.loads(text)
    assert text.endswith("\n") and isinstance(valid, dict) and "format_version" in valid
    assert text == json.dumps(valid, indent=2 if text.startswith("{\n  ") else 1, sort_keys=True) + "\n"
    read(folder)                                                        # the valid record is read

    damage = {"not JSON": b"{nope", "not UTF-8": b"\xff\xfe{}\n", "not an object": b"[1, 2]\n",
              "another version": json.dumps(dict(valid, format_version=99)).encode()}
    if exact:
        damage["an unknown field"] = json.dumps(dict(valid, surplus=1)).encode()
    for what, data in damage.items():
        with open(path, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError) as e:
            read(folder)
        assert str(e.value).startswith(path + ":"), (what, str(e.value))

    os.remove(path)
    if missing is MISSING_IS_AN_ERROR:
        with pytest.raises(ValueError) as e:
            read(folder)
        assert str(e.value).startswith(path + ": missing"), str(e.value)
    else:
        assert read(folder) == missing


def test_is_int_and_a_missing_file():
    assert [pmctf_records.is_int(v) for v in (0, -3, 2 ** 40, True, 1.0, "1", None)] == [True, True, True, False, False, False,
                                                                                         False]
    assert pmctf_records.read_record("/nonexistent/folder/x.json", "record", 1) is None
