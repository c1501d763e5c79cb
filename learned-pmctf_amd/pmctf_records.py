"""The sidecar records of a bitstream folder (sequence.json, picture_format.json, picture_hashes.json, gop_structure.json,
rate_control.json, layer_hashes.json, spatial_hashes.json, layer_extract.json, display_format.json, source_format.json):
the one place that reads and writes them as JSON.  Every record is an object with a "format_version"; what its other fields mean is checked
by the module that owns it.  Standard library only."""
import json


def is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def write_record(path, record, indent):
    """record -> path as JSON with sorted keys and a final newline -> path"""
    with open(path, "w") as f:
        json.dump(record, f, indent=indent, sort_keys=True)
        f.write("\n")
    return path


def read_record(path, what, version, fields=None, missing=None, expected=None, reader="decoder"):
    """-> the JSON value of path.  what: the record's name in "{path}: not a {what} (...)", raised for a file that is not
    JSON or not UTF-8.  A file that is not there: a ValueError "{path}: missing ({missing})" when missing is a text, else
    None is returned.  version: the one format_version read (a value that is no object has none); None: the caller checks
    the version, and the kind of value, itself.  fields: the names the record holds beside format_version, exactly; the
    message lists the record's fields and `expected` where that is given, else the missing and the unknown ones."""
    try:
        with open(path) as f:
            record = json.load(f)
    except FileNotFoundError:
        if isinstance(missing, str):
            raise ValueError(f"{path}: missing ({missing})") from None
        return None
    except (json.JSONDecodeError, UnicodeDecodeError) as e:
        raise ValueError(f"{path}: not a {what} ({e})") from None
    if version is not None and (not isinstance(record, dict) or record.get("format_version") != version):
        got = record.get("format_version") if isinstance(record, dict) else None
        raise ValueError(f"{path}: format version {got!r}, this {reader} reads version {version}")
    if fields is not None:
        check_fields(path, record, fields, expected)
    return record


def check_fields(path, record, fields, expected=None):
    """ValueError unless the record holds format_version and `fields`, exactly"""
    want = set(fields) | {"format_version"}
    if set(record) != want:
        if expected is not None:
            raise ValueError(f"{path}: fields {sorted(record)}, expected {expected}")
        raise ValueError(f"{path}: fields missing {sorted(want - set(record))}, unknown {sorted(set(record) - want)}")
