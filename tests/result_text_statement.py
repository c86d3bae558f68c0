"""The rule of the result text (include/gomatching_hip.h, `gom_result_text_*`) in plain Python, template by template: what
`results.write_video_results` / `VideoResultWriter` write between the files' header and footer, frame by frame.  No json, no
minidom, no numpy: strings and integers only.  Rows are `results.frame_lines`' rows: 8 points, the id, the transcription and
(11 elements) a segmentation of rings of [x, y] pairs of any length; a 10-element row has no "segmentation" key."""

JSON_HEADER, JSON_FOOTER, JSON_EMPTY = "{\n", "\n}", "{}"
XML_DECLARATION = '<?xml version="1.0" ?>\n'
XML_HEADER, XML_FOOTER = XML_DECLARATION + "<Frames>\n", "</Frames>\n"

_JSON_SHORT = {'"': '\\"', "\\": "\\\\", "\n": "\\n", "\r": "\\r", "\t": "\\t", "\b": "\\b", "\f": "\\f"}
_XML_ATTR = {"&": "&amp;", "<": "&lt;", '"': "&quot;", ">": "&gt;"}


def json_char(ch):
    """One character inside a JSON string, ensure_ascii=False: the short escapes, \\u00XX below U+0020, itself otherwise."""
    if ch in _JSON_SHORT:
        return _JSON_SHORT[ch]
    return "\\u%04x" % ord(ch) if ord(ch) < 0x20 else ch


def xml_char(ch):
    """One character inside an attribute value as minidom writes it."""
    return _XML_ATTR.get(ch, ch)


def integer(v):
    """Plain decimal, '-' in front of a negative value (no str(): digit by digit, as the kernel does)."""
    v = int(v)
    m, digits = abs(v), ""
    while True:
        digits = "0123456789"[m % 10] + digits
        m //= 10
        if m == 0:
            break
    return ("-" if v < 0 else "") + digits


def _sp(k):
    return " " * k


def _ring(ring, depth):
    """A list of [x, y] pairs at `depth` spaces; an empty ring is `[]`, as an empty pair would be."""
    if not ring:
        return _sp(depth) + "[]"
    pairs = []
    for pair in ring:
        if not pair:
            pairs.append(_sp(depth + 4) + "[]")
            continue
        pairs.append(_sp(depth + 4) + "[\n" + ",\n".join(_sp(depth + 8) + integer(v) for v in pair) + "\n" + _sp(depth + 4) + "]")
    return _sp(depth) + "[\n" + ",\n".join(pairs) + "\n" + _sp(depth) + "]"


def row_json(row):
    out = _sp(8) + "{\n"
    out += _sp(12) + '"points": [\n' + ",\n".join(_sp(16) + integer(v) for v in row[:8]) + "\n" + _sp(12) + "],\n"
    out += _sp(12) + '"ID": ' + integer(row[8]) + ",\n"
    out += _sp(12) + '"transcription": "' + "".join(json_char(c) for c in row[9]) + '"'
    if len(row) == 11:
        rings = row[10]
        out += ",\n" + _sp(12) + '"segmentation": '
        out += "[]" if not rings else "[\n" + ",\n".join(_ring(r, 16) for r in rings) + "\n" + _sp(12) + "]"
    return out + "\n" + _sp(8) + "}"


def frame_json(f, rows):
    """Frame f (0-based, written under the key f + 1) of the JSON stream."""
    out = (",\n" if f else "") + _sp(4) + '"' + integer(f + 1) + '": '
    if not rows:
        return out + "[]"
    return out + "[\n" + ",\n".join(row_json(r) for r in rows) + "\n" + _sp(4) + "]"


def row_xml(row):
    out = _sp(4) + '<object ID="' + integer(row[8]) + '" Transcription="' + "".join(xml_char(c) for c in row[9]) + '">\n'
    for i in range(4):
        out += _sp(6) + '<Point x="' + integer(row[2 * i]) + '" y="' + integer(row[2 * i + 1]) + '"/>\n'
    return out + _sp(4) + "</object>\n"


def frame_xml(f, rows):
    """Frame f of the XML stream."""
    if not rows:
        return _sp(2) + '<frame ID="' + integer(f + 1) + '"/>\n'
    return _sp(2) + '<frame ID="' + integer(f + 1) + '">\n' + "".join(row_xml(r) for r in rows) + _sp(2) + "</frame>\n"


def video_json(frames):
    """The whole JSON file of a video whose frame i has the rows frames[i]."""
    if not frames:
        return JSON_EMPTY
    return JSON_HEADER + "".join(frame_json(f, rows) for f, rows in enumerate(frames)) + JSON_FOOTER


def video_xml(frames):
    if not frames:
        return XML_DECLARATION
    return XML_HEADER + "".join(frame_xml(f, rows) for f, rows in enumerate(frames)) + XML_FOOTER
