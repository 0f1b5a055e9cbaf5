"""Command-line entry points; option helpers they share."""


def quantize_choice(value: str):
    """argparse type of the CLIs' --quantize: 4, 8 or fp8."""
    if value == "fp8":
        return "fp8"
    if value in ("4", "8"):
        return int(value)
    import argparse
    raise argparse.ArgumentTypeError(
        f"invalid choice: {value!r} (choose from 4, 8, fp8)")


def quantize_request(choice, group_size: int):
    """load_model's ``quantize`` argument from the CLI options
    (--quantize-group-size is ignored for fp8)."""
    if not choice:
        return None
    return "fp8" if choice == "fp8" else (choice, group_size)
